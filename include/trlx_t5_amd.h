/*
 * trlx_t5_amd.h — C ABI of the MI355X-native PPO experience-and-loss hot path.
 *
 * Test-free, torch-free boundary: plain device pointers, int64 sizes/strides (in
 * ELEMENTS), dtype enums, scalar hyper-parameters by value and the caller's stream
 * (a hipStream_t passed as void*; NULL = the default stream).  Every entry point is
 * stream-ordered and asynchronous: no host synchronisation, no allocation, no pointer
 * retained past the call.  All return an int status (TRLX_OK = 0); on failure
 * trlx_last_error() returns a thread-local message.
 *
 * The reference (danyang-rainbow/trlx-t5) has no FFI layer: its hot path is plain
 * Python functions.  Each entry point below names the reference function (file:line,
 * into the reference repo) whose arithmetic it replaces; the Python drop-in that binds
 * them (trlx-t5_amd/) keeps those functions' names and signatures.
 *
 * Layout conventions
 *   logits   : [B, T, V], row (b, t) starts at  logits + b*sb + t*st,  V contiguous.
 *   labels   : int64, element (b, t) at labels + b*lb + t*lt, in [0, V) (out of range
 *              produces NaN, never an out-of-bounds read).
 *   [B, T] per-token vectors (logprobs, values, rewards, advantages, ...) : contiguous.
 *   dtype    : TRLX_F32 or TRLX_BF16 (logits / per-token vectors), arithmetic is fp32
 *              with fp64 accumulation for batch statistics.
 */
#ifndef TRLX_T5_AMD_H
#define TRLX_T5_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRLX_ABI_VERSION 2

typedef enum {
    TRLX_F32 = 0,
    TRLX_BF16 = 1,
    TRLX_I64 = 2,   /* masks / lengths only */
} trlx_dtype;

typedef enum {
    TRLX_OK = 0,
    TRLX_ERR_SHAPE = 1,   /* bad size / shape */
    TRLX_ERR_STRIDE = 2,  /* unsupported stride */
    TRLX_ERR_DTYPE = 3,   /* unsupported dtype */
    TRLX_ERR_LAUNCH = 4,  /* kernel launch failed */
    TRLX_ERR_ARG = 5,     /* NULL pointer / bad scalar */
} trlx_status;

/* Number of fp64 slots per partial-statistics record (see trlx_gae_scan). */
#define TRLX_MOMENT_SLOTS 4     /* {sum x, sum x^2, count, sum mask} */
#define TRLX_SPLIT_MOMENT_SLOTS 8 /* {Σ A0, Σ A0², n, Σ Ak, Σ A0·Ak, Σ Ak², Σ mask, 0} */
/* Number of fp32 slots written by trlx_ppo_loss_finalize (order = stats keys of
 * PPOConfig.loss, ppo_models.py:182-198, after losses). */
#define TRLX_PPO_STATS 13
/* Number of fp64 partial-sum slots per block of trlx_ppo_loss_elem. */
#define TRLX_PPO_PARTIAL_SLOTS 16

int trlx_abi_version(void);
const char* trlx_last_error(void);

/* Launch tuning for A/B measurements (0 = automatic, the default).  The values are
 * thread-local: they steer only the launches issued by the calling host thread, so one
 * thread's experiment never changes another thread's kernels or summation order.  Keys:
 *   "row_variant"       1 = register-resident vocab rows, 2 = streaming vocab rows
 *   "resident_threads"  workgroup size for resident rows (multiple of 64)
 *   "resident_lb512"    1 = <=512-thread resident rows compiled for 8 waves/SIMD (default 0; always on
 *                       for forward rows of <= 8 vectors per thread)
 *   "stream_threads"    workgroup size for streaming rows
 *   "stream_unroll"     16-B loads in flight per thread for streaming rows (2, 4, 8)
 *   "row_order"         resident rows: 0 (default) = step-major vectors, 1 = wave-major
 *   "split_lds"         long rows (fp32 V > 32 k, bf16 V > 32 k): 0 = split VGPR + LDS residency
 *                       for the loss / backward (default), 1 = off, 2 = also for the forward
 *   "ilql_split"        ILQL fp32 rows in split residency (8192 < V/4 + 16 <= 12800; off with split_lds = 1):
 *                       VGPR + LDS vector steps 0 = 20 + 5 (default), 1 = 22 + 3, 2 = 21 + 4, 3 = 19 + 6
 *   "split_mid"         mid-length bf16 rows (16k < V <= 32k) in the loss / backward: 0 auto (= 3),
 *                       1 = all in VGPRs, 2 = 5 VGPR + 3 LDS vector steps, 3 = 6 + 2 (8 waves/SIMD)
 *   "ragged_order"      ragged experience rows with an order scratch: 0 = valid rows first (default),
 *                       1 = natural order
 *   "order_launch"      the valid-rows-first order: 0 auto (one launch up to 64 chunks of 1024 rows,
 *                       then two), 1 = one launch, 2 = two chunk-count launches
 *   "lmloss_splits"     fused loss forward vocab splits: 0 auto (the fullest last round), 1..8 fixed
 *   "lmloss_dw_tsplit"  fused loss dW: 0 auto (the last round's vocab blocks split over the tokens),
 *                       1 = no split, 2..16 = that many token splits
 *   "lmloss_fwd"        fused loss forward form: 0 / 2 = the 16x16x32 form (the only one built; the
 *                       removed forms 1, 3, 4 are rejected with TRLX_ERR_ARG)
 *   "lmloss_dw"         fused loss dW plan: 0 auto (saved P where the caller's buffers hold it),
 *                       1 = recompute S (k_lmloss_dw), 4 = saved P (k_lmloss_dwp); 2, 3 rejected
 *   "lmloss_dwp_form"   saved-P dW blocking: 0 auto (= 2: 32 rows a wave x H/2), 1 = 16 rows a wave x H
 *   "store_policy"      gradient-row store cache policy: 0 auto (default: nt; sc1 for all-VGPR rows
 *                       launches writing > 1.5 GB), 1 none, 2 sc1, 3 sc0|sc1, 4 nt|sc1, 5 nt
 *   "vhead_splits"      value head column splits: 0 auto (trlx_value_head_splits), 1..64 fixed (capped
 *                       at one split per 32 columns)
 * Results are identical up to fp32 summation order; only speed changes. */
int trlx_set_tuning(const char* key, int64_t value);

/* ---------------------------------------------------------------- A1
 * logprobs_from_logits forward — replaces trlx/utils/modeling.py:37-41
 * (F.log_softmax over V + gather at labels), fused in one pass over each row; the
 * [B,T,V] log-softmax is never materialised.
 * Up to two logits tensors of identical shape/strides/dtype are processed in one launch
 * (x1 may be NULL): the experience step's policy and reference logits
 * (ppo_orchestrator.py:154-155).  out_lp{0,1}: [B,T] of out_dtype.  out_lse{0,1}:
 * optional fp32 [B,T] log-sum-exp saved for the backward. */
int trlx_lsm_gather_fwd(const void* x0, const void* x1, int dtype,
                        int64_t B, int64_t T, int64_t V, int64_t sb, int64_t st,
                        const int64_t* labels, int64_t lb, int64_t lt,
                        void* out_lp0, void* out_lp1, int out_dtype,
                        float* out_lse0, float* out_lse1, void* stream);
/* The experience rows of a ragged batch (decoder lengths [B] int64): a row (b, t) with
 * t >= lengths[b] is store padding — ppo_pipeline.py:47-65 pads each element's logprobs with
 * 0.0 — so its lp is 0 and the row is NOT read (the bytes of a batch of decoder lengths L_b
 * are those of its sum(L_b) tokens).  lengths == NULL: trlx_lsm_gather_fwd.  order_ws (or
 * NULL): trlx_ragged_order_bytes(B, T) bytes of device scratch — a small launch
 * first orders the rows valid-first so the skipped rows do not interleave with them (the
 * scratch then holds the B·T row ids, valid first and ~id for the padding, and the count). */
int64_t trlx_ragged_order_bytes(int64_t B, int64_t T);
int trlx_lsm_gather_fwd_ragged(const void* x0, const void* x1, int dtype,
                               int64_t B, int64_t T, int64_t V, int64_t sb, int64_t st,
                               const int64_t* labels, int64_t lb, int64_t lt, const int64_t* lengths,
                               void* order_ws, void* out_lp0, void* out_lp1, int out_dtype, void* stream);

/* ---------------------------------------------------------------- A1 backward
 * Autograd of modeling.py:39-40 (log_softmax_backward of the gathered one-hot):
 *   dx[b,t,j] = g[b,t] * ([j == y] - exp(x[b,t,j] - lse[b,t]))
 * grad: [B,T] of grad_dtype; dx row (b,t) at dx + b*dsb + t*dst, same dtype as x.  One
 * read of the row and one write, no reduction (lse from the forward). */
int trlx_lsm_gather_bwd(const void* x, int dtype, int64_t B, int64_t T, int64_t V,
                        int64_t sb, int64_t st, const int64_t* labels, int64_t lb, int64_t lt,
                        const float* lse, const void* grad, int grad_dtype,
                        void* dx, int64_t dsb, int64_t dst, void* stream);

/* ---------------------------------------------------------------- A2
 * KL-penalised reward — replaces ppo_orchestrator.py:164-167:
 *   r[b,t] = -beta * (lp[b,t] - ref_lp[b,t]);  r[b, T-1] += scores[b]
 * (with lengths != NULL the score goes to column lengths[b]-1 and columns >= lengths[b]
 * are padding: reward 0).  lp/ref_lp: [B,T] of in_dtype; scores fp32 [B] or NULL. */
int trlx_kl_penalty_rewards(const void* lp, const void* ref_lp, int in_dtype,
                            int64_t B, int64_t T, float beta, const float* scores,
                            const int64_t* lengths, void* rewards, int out_dtype, void* stream);

/* ---------------------------------------------------------------- A5 (+A2 fused, +A3 partials)
 * GAE reverse scan — replaces ppo_models.py:121-136 (the per-t Python loop):
 *   delta_t = r_t + gamma*V_{t+1} - V_t   (V_T := 0);   A_t = delta_t + (gamma*lam)*A_{t+1}
 *   returns = A + V  (unwhitened A)
 * values / rewards: [B, T] of dtype (rows contiguous, row stride T); columns
 * [0, Teff) are used (Teff = response_length).  If lp != NULL the rewards are not read
 * but computed in-kernel from (lp, ref_lp, neg_beta, scores) exactly as
 * trlx_kl_penalty_rewards does (fp32 lp/ref_lp [B,T]) and, if rew_out != NULL, stored.
 * lengths (nullable): positions t >= lengths[b] are padding (value/reward read as 0).
 * Outputs: adv_raw fp32 [B,Teff] (unwhitened), ret [B,Teff] of ret_dtype, and per-block
 * partial moments of adv_raw: partials[blk*4 + {0,1,2,3}] = {sum A, sum A^2, count,
 * sum mask} (mask: int64 [B,Teff] loss mask, NULL = all ones).
 * trlx_gae_num_blocks(B, Teff) tells how many partial records are written.  With
 * stats != NULL the last block to finish also reduces them (fixed order) into stats[4];
 * `ticket` is then a device uint32 that must be 0 before the first call (the kernel
 * re-arms it).
 * gamma and lam are doubles (here and in every entry that takes them): the reference
 * multiplies the two Python floats and the product meets fp32 tensors, so the kernels use
 * fl32(gamma) and fl32(gamma*lam), each rounded once; fp32 arguments would round the factors
 * before the product and move it by an ulp for e.g. (0.99, 0.99).
 * One workgroup scans up to 16 rows staged in LDS; the rows per block shrink with Teff so
 * that the launch's whole LDS (dynamic + static) stays within 64 KiB, and a Teff whose single
 * row does not fit (Teff > 8172) is refused with TRLX_ERR_SHAPE. */
int64_t trlx_gae_num_blocks(int64_t B, int64_t Teff);
int trlx_gae_scan(const void* values, const void* rewards, int dtype, int64_t B, int64_t T,
                  int64_t Teff, double gamma, double lam,
                  const float* lp, const float* ref_lp, float neg_beta, const float* scores,
                  const int64_t* lengths, const int64_t* mask,
                  float* adv_raw, void* ret, int ret_dtype, void* rew_out, int rew_dtype,
                  double* partials, double* stats, unsigned* ticket, void* stream);

/* ---------------------------------------------------------------- A3 helpers
 * Partial moments of an arbitrary contiguous tensor (for whiten / get_global_statistics,
 * modeling.py:9-34, and RunningMoments, :72-104).  trlx_moments_num_blocks(n) records. */
int64_t trlx_moments_num_blocks(int64_t n);
int trlx_moments_partial(const void* x, int dtype, int64_t n, double* partials, void* stream);
/* (dtype may also be TRLX_I64 here, e.g. to sum a loss mask.) */
/* Reduce nblk partial records (fixed order, deterministic) into stats[4]. */
int trlx_moments_finalize(const double* partials, int64_t nblk, double* stats, void* stream);

/* ---------------------------------------------------------------- A4
 * whiten — replaces modeling.py:24-34:  out = (x - mu) * rsqrt(var + 1e-8) [+ mu]
 * mu, var from stats[4] = {sum, sumsq, count, .}: var = M2/count (biased, the
 * distributed branch) or M2/(count-1) (unbiased, torch.var_mean branch). */
int trlx_whiten_apply(const void* x, int dtype, int64_t n, const double* stats, int unbiased,
                      int shift_mean, void* out, int out_dtype, void* stream);

/* ---------------------------------------------------------------- A1+A4+A6 fused (loss side)
 * One pass over each policy-logits row: lse, lp = x[y] - lse, then the closed-form
 * per-token gradient of PPOConfig.loss's policy term (ppo_models.py:165-177 with torch's
 * max-tie and clamp-bound rules) and the row's dlogits = g * (onehot - softmax), written
 * once.  Advantages are whitened on the fly from adv_raw + stats (stats == NULL: adv is
 * used as given).  mask: int64 [B,T] or NULL (all ones); msum: device fp64 scalar (NULL:
 * use msum_host).  Outputs: lp_out fp32 [B,T]; dx (row (b,t) at dx + b*dsb + t*dst, dtype
 * of x).  A masked token (mask == 0) has d loss / d lp = 0 exactly, so its dlogits row is
 * written as zeros WITHOUT reading its logits and lp_out is 0 there (for every loss-rows
 * entry point below as well; the token's loss terms are those of any finite lp). */
int trlx_ppo_policy_fused(const void* x, int dtype, int64_t B, int64_t T, int64_t V,
                          int64_t sb, int64_t st, const int64_t* labels, int64_t lb, int64_t lt,
                          const void* old_lp, int old_dtype, const float* adv,
                          const double* stats, int unbiased, const int64_t* mask,
                          const double* msum, double msum_host, float cliprange,
                          float* lp_out, void* dx, int64_t dsb, int64_t dst, void* stream);

/* ---------------------------------------------------------------- the fused step (2 launches)
 * Experience: policy + reference rows -> lp, ref_lp (fp32); then one wavefront per rollout
 * computes its KL-penalised rewards, GAE advantages (unwhitened, fp32) and returns, and the
 * last block the whitening moments stats[4] = {Σ A, Σ A², n, Σ mask}.  Replaces ppo_orchestrator.py:
 * 154-167 followed by ppo_models.py:121-136 (+ the moments of modeling.py:24-29).
 * Loss: new-policy rows -> lp_out, dlogits (one read + one write), the value-loss gradient
 * dvalues and per-token loss terms; then one wavefront per rollout sums them and the last
 * block writes loss[1] + loss_stats[13] (order of trlx_ppo_loss_finalize),
 * i.e. ppo_models.py:141-199 with its autograd into the logits.  `stats` (possibly
 * all-reduced across ranks in between) whitens the advantages on the fly; unbiased as in
 * trlx_whiten_apply.  workspace: trlx_ppo_workspace_bytes(B, T) bytes, zero-filled once
 * before the first use and then reusable (the kernels re-arm their tickets).  Rows (b, t)
 * of the rollout batch must be contiguous rollouts (t fastest).  With lengths, the
 * experience rows past each rollout's length are store padding (lp = ref_lp = 0, not read:
 * trlx_lsm_gather_fwd_ragged); with a mask, the loss rows of masked tokens are not read
 * (trlx_ppo_policy_fused). */
int64_t trlx_ppo_workspace_bytes(int64_t B, int64_t T);
int trlx_ppo_experience_fused(const void* logits, const void* ref_logits, int dtype, int64_t B, int64_t T,
                              int64_t V, int64_t sb, int64_t st, const int64_t* labels, int64_t lb,
                              int64_t lt, const void* values, int v_dtype, const float* scores,
                              const int64_t* lengths, const int64_t* mask, float kl_coef, double gamma,
                              double lam, float* lp, float* ref_lp, float* rewards, float* adv_raw,
                              void* ret, int ret_dtype, double* stats, void* workspace, void* stream);
/* The two launches of each fused entry point, separately (same arguments):
 *   experience = trlx_lsm_gather_fwd_ragged(policy, ref -> fp32 lp, ref_lp) + trlx_ppo_rollout_gae
 *   loss       = trlx_ppo_loss_rows + trlx_ppo_rollout_loss  */
int trlx_ppo_rollout_gae(int64_t B, int64_t T, const float* lp, const float* ref_lp, const void* values,
                         int v_dtype, const float* scores, const int64_t* lengths, const int64_t* mask,
                         float kl_coef, double gamma, double lam, float* rewards, float* adv_raw, void* ret,
                         int ret_dtype, double* stats, void* workspace, void* stream);
int trlx_ppo_loss_rows(const void* logits, int dtype, int64_t B, int64_t T, int64_t V, int64_t sb, int64_t st,
                       const int64_t* labels, int64_t lb, int64_t lt, const void* old_lp, int old_dtype,
                       const float* adv_raw, const double* stats, int unbiased, const int64_t* mask,
                       const void* values, int v_dtype, const void* old_values, int ov_dtype,
                       const void* returns, int r_dtype, float cliprange, float cliprange_value, float vf_coef,
                       float* lp_out, void* dx, int64_t dsb, int64_t dst, float* dvalues, void* workspace,
                       void* stream);
int trlx_ppo_rollout_loss(int64_t B, int64_t T, const double* stats, float vf_coef, float* loss,
                          float* loss_stats, void* workspace, void* stream);
int trlx_ppo_loss_fused(const void* logits, int dtype, int64_t B, int64_t T, int64_t V, int64_t sb,
                        int64_t st, const int64_t* labels, int64_t lb, int64_t lt, const void* old_lp,
                        int old_dtype, const float* adv_raw, const double* stats, int unbiased,
                        const int64_t* mask, const void* values, int v_dtype, const void* old_values,
                        int ov_dtype, const void* returns, int r_dtype, float cliprange,
                        float cliprange_value, float vf_coef, float* lp_out, void* dx, int64_t dsb,
                        int64_t dst, float* dvalues, float* loss, float* loss_stats, void* workspace,
                        void* stream);

/* ---------------------------------------------------------------- A6
 * PPOConfig.loss (ppo_models.py:141-199) over [B,T] vectors.  Pass 1 (elementwise,
 * many blocks): per-token value/policy terms, gradients d loss/d lp (dlp, optional) and
 * d loss/d values (dv, optional) and fp64 partial sums (TRLX_PPO_PARTIAL_SLOTS per
 * block).  Pass 2 (one block, fixed order): loss[1] and stats[TRLX_PPO_STATS] fp32 in the
 * order total_loss, policy_loss, value_loss, mean_old_values, var_old_values,
 * mean_values, values_error, values_clipfrac, approx_kl, policy_clipfrac,
 * returns_mean, returns_var, ratio.
 * lp, values, old_lp, old_values, adv, returns: [n] of the respective dtypes (adv fp32,
 * optionally whitened on the fly from adv_stats); mask int64 [n] or NULL. */
int64_t trlx_ppo_loss_num_blocks(int64_t n);
int trlx_ppo_loss_elem(int64_t n, const void* lp, int lp_dtype, const void* values, int v_dtype,
                       const void* old_lp, int olp_dtype, const void* old_values, int ov_dtype,
                       const void* adv, int a_dtype,
                       const double* adv_stats, int unbiased, const void* returns,
                       int r_dtype, const int64_t* mask, const double* msum, double msum_host,
                       float cliprange, float cliprange_value, float vf_coef,
                       void* dlp, void* dv, int g_dtype, double* partials,
                       float* loss, float* stats, unsigned* ticket, void* stream);
/* (with ticket != NULL — a device uint32, 0 before the first call — the last block of
 *  trlx_ppo_loss_elem performs pass 2 itself: one launch for the whole loss.) */
int trlx_ppo_loss_finalize(const double* partials, int64_t nblk, int64_t n,
                           const double* msum, double msum_host, float vf_coef,
                           float* loss, float* stats, void* stream);

/* ---------------------------------------------------------------- A10 (ILQL loss)
 * ILQLConfig.loss — replaces trlx/model/nn/ilql_models.py:52-116 with its autograd
 * (config 5).  Every vocab row (logits [B,L,V] and the nq Q-head rows [B,A,V]) is read
 * once into registers and its gradient row written once:
 *   logits row (b,t<L-1): CE against input_ids[b,t+1], weight attention_mask[b,t+1]
 *                         (AWAC, :98-105); row t = L-1 gets a zero gradient
 *   q_i row (b,a)       : CE against the action a* = input_ids[b, 1+actions_ixs[b,a]]
 *                         weighted by dones[b,a] (CQL, :87-96) + the TD term
 *                         ((Q_i[a*] - (r + gamma*vs[b,a+1]*dones[b,a+1]))*dones[b,a])^2 (:63-74)
 *   target-Q rows are only gathered at a* (min over heads) for the expectile V loss (:76-83);
 *   with tq_gathered = 1 the caller passes the values at a* themselves.
 * Three launches: prep (n_nonterminal = max(1, sum dones[:, :-1]) and sum attention[:, 1:]),
 * rows (one workgroup per vocab row), finalize (fixed-order fp64 sums -> losses[5] =
 * {loss, loss_q, loss_v, loss_cql, loss_awac}); prep and finalize run a few workgroups whose
 * last reduces the block records in fixed order (an arrival ticket in the workspace).  dvs = d loss / d vs (fp32 [B, A+1], last
 * column 0).  Gradient rows have the same strides and 16-B phase as their inputs.  The
 * small [B, .] tensors are contiguous.  No collective: the reference's ILQL loss is
 * rank-local (DDP averages the gradients). */
typedef struct {
    int dtype;                        /* TRLX_F32 / TRLX_BF16: logits, q, tq rows */
    int nq;                           /* 1 or 2 Q heads (ILQLConfig.two_qs) */
    int64_t B, L, A, V;               /* rows, tokens, actions (states = A + 1), vocab */
    const void* logits;               /* [B,L,V], row (b,t) at logits + b*logits_sb + t*logits_st */
    int64_t logits_sb, logits_st;
    const void* q[2];                 /* [B,A,V] Q heads (q[1] unused when nq == 1) */
    int64_t q_sb[2], q_st[2];
    const void* tq[2];                /* [B,A,V] target Q heads (gathered only); see tq_gathered */
    int64_t tq_sb[2], tq_st[2];
    const int64_t* input_ids;         /* [B,L] */
    const int64_t* attention_mask;    /* [B,L] */
    const int64_t* actions_ixs;       /* [B,A] */
    const int64_t* dones;             /* [B,A+1] */
    const void* rewards;              /* [B,A] */
    int rewards_dtype;
    const void* vs;                   /* [B,A+1] (the reference's [B,S,1]) */
    int vs_dtype;
    float tau, gamma, cql_scale, awac_scale;
    void* dlogits;                    /* gradient rows, dtype of the inputs */
    int64_t dlogits_sb, dlogits_st;
    void* dq[2];
    int64_t dq_sb[2], dq_st[2];
    float* dvs;                       /* [B,A+1] fp32 */
    float* losses;                    /* [5] fp32 */
    void* workspace;                  /* trlx_ilql_workspace_bytes(B, L, A, nq) bytes, zero-filled
                                         once before first use (prep / finalize re-arm their tickets) */
    int tq_gathered;                  /* 0: tq[i] are [B,A,V] rows of `dtype`, gathered at a* here.
                                         1: tq[i] are fp32 [B,A] values already taken at a*
                                         (trlx_ilql_tq_at_actions): element (b,a) at
                                         tq[i] + b*tq_sb[i] + a*tq_st[i]; `dtype` does not describe
                                         them; an a* outside [0, V) still makes the value NaN */
} trlx_ilql_args;

int64_t trlx_ilql_workspace_bytes(int64_t B, int64_t L, int64_t A, int nq);
int trlx_ilql_prep(const trlx_ilql_args* args, void* stream);
int trlx_ilql_rows(const trlx_ilql_args* args, void* stream);
int trlx_ilql_finalize(const trlx_ilql_args* args, void* stream);
int trlx_ilql_loss_fused(const trlx_ilql_args* args, void* stream);   /* the three in order */

/* ---------------------------------------------------------------- ILQL heads
 * The target-Q heads at the action tokens only — replaces the second Linear of
 * `target_qs = tuple(q_head(actions_hs) for q_head in self.target_q_heads)`
 * (ilql_models.py:31-34,156) for the loss, which reads tq_i[b, a, a*] alone
 * (a* = input_ids[b, 1 + actions_ixs[b, a]], computed here exactly as the loss rows do):
 *   out[i][b, a] = sum_k z[i][b, a, k] * w2[i][a*, k] + b2[i][a*]
 * z[i]: the head's post-ReLU hidden activations [B, A, K], element (b, a, k) at
 * z[i] + b*z_sb[i] + a*z_st[i] + k; w2[i]: [V, K] (nn.Linear layout), rows of w2_ld[i]
 * elements; b2[i]: [V] or NULL; all of `dtype` (TRLX_F32 / TRLX_BF16).  out[i]: fp32 [B, A],
 * contiguous.  One launch for nh = 1 or 2 heads, one wave per (token, head).  fp32
 * accumulation in an order fixed by (K, dtype) alone: bit-reproducible, independent of B, A,
 * the grid and the rows' alignment (16-B loads when K is a multiple of the vector width and
 * both rows are 16-B aligned, element loads into the same chains otherwise).  Any K >= 1.
 * An a* outside [0, V) (or actions_ixs outside [0, L-1)) gives NaN and reads nothing. */
typedef struct {
    int dtype;                        /* TRLX_F32 / TRLX_BF16: z, w2, b2 */
    int nh;                           /* 1 or 2 heads */
    int64_t B, L, A, K, V;
    const void* z[2];
    int64_t z_sb[2], z_st[2];
    const void* w2[2];
    int64_t w2_ld[2];
    const void* b2[2];                /* or NULL */
    const int64_t* input_ids;         /* [B,L] */
    const int64_t* actions_ixs;       /* [B,A] */
    float* out[2];                    /* [B,A] fp32 */
} trlx_ilql_tq_args;
int trlx_ilql_tq_at_actions(const trlx_ilql_tq_args* args, void* stream);

/* Polyak sync of the target heads — replaces ILQLHeads._sync_target_q_heads
 * (ilql_models.py:161-168): for each of `count` tensors of one dtype (TRLX_F32 / TRLX_BF16)
 *   target[i][k] = (alpha * src[i][k]) + (1 - alpha) * target[i][k],   k < numel[i]
 * rounded as torch's three elementwise ops: alpha and 1.0 - alpha (formed in double) are
 * each rounded to fp32, every product is rounded separately (no fma), and for bf16 each
 * product and the sum are rounded to bf16.  The (src, target, numel) triples travel to the
 * kernel by value, TRLX_POLYAK_MAX_TENSORS per launch; a longer list is split into several
 * launches.  The host arrays are read during the call only.  Zero-length tensors are
 * skipped; any element alignment and any tail length; a source that overlaps its target is
 * refused with TRLX_ERR_ARG (before anything is launched). */
#define TRLX_POLYAK_MAX_TENSORS 16
int trlx_polyak_update(const void* const* src, void* const* target, const int64_t* numel, int64_t count,
                       int dtype, double alpha, void* stream);

/* ---------------------------------------------------------------- fused multi-tensor AdamW
 * The three lines every update of the reference ends with (accelerate_base_model.py:94-106,
 * 263-265: opt.step() of torch.optim.AdamW) and, for ILQL, the Polyak sync of
 * post_backward_callback in the same pass.  For each of `count` tensors, element by element in
 * fp32, in the order of torch's _single_tensor_adam with decoupled decay, every op rounded
 * separately (no fma):
 *   p = p * (1 - lr*wd)
 *   m = m + (1-b1) * (g - m)
 *   v = v*b2 + (1-b2) * (g*g)
 *   p = p + (-(lr/bc1)) * (m / (sqrt(v)/sqrt(bc2) + eps))      bc1 = 1 - b1^step, bc2 = 1 - b2^step
 * The scalars 1 - lr*wd, 1-b1, b2, 1-b2, -(lr/bc1), sqrt(bc2) and eps are formed in double
 * by this call and rounded to fp32 once.  step >= 1 is the number of the update being made.
 *   p      : p_dtype (TRLX_F32 / TRLX_BF16), in/out.
 *   g      : g_dtype (TRLX_F32 / TRLX_BF16).          m, v : fp32, in/out.
 *   master : NULL array, or per tensor NULL or an fp32 copy of a bf16 p: the master is what is
 *            updated and p is written as the master rounded to bf16 (round-to-nearest-even).
 *            Without it a bf16 p is upcast, updated in fp32 and rounded to bf16 once.  A master
 *            for an fp32 p is refused.
 *   target : NULL array, or per tensor NULL or a tensor of p_dtype that receives
 *              target = (alpha * p_new) + (1 - alpha) * target
 *            rounded exactly as trlx_polyak_update rounds it (bf16 form included), where p_new
 *            is the value stored to p (for bf16 the rounded one).
 * The pointers travel to the kernel by value, TRLX_ADAMW_MAX_TENSORS tensors per launch; a
 * longer list is split into several launches.  One workgroup takes TRLX_ADAMW_CHUNK elements
 * of one tensor.  16-byte loads and stores wherever all pointers of a tensor share a 16-byte
 * phase (one head of fewer than 8 elements brings every one of them to a 16-byte boundary),
 * element accesses otherwise: any element alignment, any tail length; the result bits do not
 * depend on the path.  Zero-length tensors are skipped.  The host arrays are read during the
 * call only.  Refused before anything is launched: a NULL pointer in a live entry
 * (TRLX_ERR_ARG), a dtype other than the above (TRLX_ERR_DTYPE), a pointer not aligned to its
 * element size (TRLX_ERR_ARG), any overlap among p, g, m, v, master and target of one entry
 * (TRLX_ERR_ARG), a tensor of more than TRLX_ADAMW_CHUNK * 2^30 elements (TRLX_ERR_SHAPE),
 * step < 1 or a NaN scalar (TRLX_ERR_ARG). */
#define TRLX_ADAMW_MAX_TENSORS 32
#define TRLX_ADAMW_CHUNK 8192
typedef struct {
    int p_dtype, g_dtype;
    int64_t count;
    void* const* p;
    const void* const* g;
    void* const* m;
    void* const* v;
    void* const* master;              /* NULL = no tensor has one */
    void* const* target;              /* NULL = no tensor has one */
    const int64_t* numel;
    int64_t step;
    double lr, beta1, beta2, eps, weight_decay;
    double alpha;                     /* read only where a target is given */
    const void* lr_table;             /* read by the _dev entries only (below): the device fp64 table that */
    int64_t n_lr;                     /* trlx_adamw_advance reads for this record, or NULL / 0: not given */
} trlx_adamw_args;
int trlx_adamw_step(const trlx_adamw_args* args, void* stream);

/* ---------------------------------------------------------------- global-norm gradient clipping
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2.0) — what DeepSpeed's
 * `gradient_clipping: 1.0` does before every update of the reference — as a device record that
 * the AdamW step reads, so the clip costs one more read of the gradients and no host sync:
 *   sumsq = Σ over all tensors Σ g²              every square and every sum in fp64, fixed order
 *   norm  = float(sqrt(sumsq))
 *   coef  = min(max_norm * (1 / (norm + 1e-6)), 1)    separately rounded fp32 ops (torch evaluates
 *           `max_norm / tensor` as tensor.reciprocal() * max_norm); a NaN stays NaN;
 *           max_norm = +inf records the norm only: coef = 1
 *   g'    = g * coef                              fp32 product; for a bf16 g, coef is first rounded to
 *           bf16 and the product rounded back to bf16: what torch's g.mul_(coef) with a 0-d device
 *           tensor (and its _foreach_mul_) computes on the device
 * trlx_grad_norm runs k_grad_sumsq (one workgroup per TRLX_ADAMW_CHUNK elements of one tensor,
 * TRLX_ADAMW_MAX_TENSORS tensors per launch, fp32 and bf16 tensors mixed, 16-byte loads from the
 * first 16-byte boundary at any element alignment and any length; one fp64 partial per workgroup
 * in `workspace`), then k_grad_norm_finish (all partials in a fixed order -> `record`), then,
 * as scale_in_place asks, k_grad_scale (g <- g' in place).  No atomics: for the same tensors at
 * the same addresses the record is bit-reproducible.  Zero-length tensors are skipped; with no
 * live tensor the record is that of an all-zero gradient.
 * trlx_adamw_step_clipped is trlx_adamw_step with every gradient element replaced by g' as it is
 * read (coef from `record`, on the device); g itself is not written.  Bit for bit it leaves what
 * trlx_grad_norm(scale_in_place = 1) followed by trlx_adamw_step leaves in p, m, v, master and
 * target.
 * Refused before anything is launched: a NULL pointer in a live entry, a NULL record or
 * workspace, a workspace smaller than trlx_grad_norm_workspace_bytes, a record not aligned to
 * 8 bytes, a gradient not aligned to its element size, a NaN or negative max_norm, a record or
 * workspace that overlaps a gradient or each other (trlx_adamw_step_clipped: a record that
 * overlaps any tensor of the step) — all TRLX_ERR_ARG; a dtype other than TRLX_F32 / TRLX_BF16
 * (TRLX_ERR_DTYPE); a negative numel or a tensor too large for the grid (TRLX_ERR_SHAPE). */
typedef struct {
    float norm;                       /* float(sqrt(sumsq)) */
    float coef;                       /* the clip coefficient, <= 1 (or NaN) */
    int32_t nonfinite;                /* 1 when norm is inf or NaN */
    int32_t pad;
    double sumsq;                     /* kept so that ranks can add theirs before the root */
    int64_t reserved;                 /* written as 0 */
} trlx_grad_norm_record;              /* 32 bytes */
typedef struct {
    int64_t count;
    const void* const* g;
    const int* g_dtype;               /* per tensor: TRLX_F32 / TRLX_BF16 */
    const int64_t* numel;
    double max_norm;                  /* >= 0, or +inf: record the norm only */
    void* record;                     /* trlx_grad_norm_record on the device, 8-byte aligned */
    void* workspace;
    int64_t workspace_bytes;
    int scale_in_place;               /* 0: record only; 1: record, then g <- g'; 2: g <- g' from a
                                         record already written (nothing else is launched) */
} trlx_grad_norm_args;
/* 8 bytes per workgroup of k_grad_sumsq (at least 8); -1 for a NULL list or a negative numel */
int64_t trlx_grad_norm_workspace_bytes(const int64_t* numel, int64_t count);
int trlx_grad_norm(const trlx_grad_norm_args* args, void* stream);
int trlx_adamw_step_clipped(const trlx_adamw_args* args, const void* record, void* stream);

/* ---------------------------------------------------------------- device-resident AdamW schedule
 * The step counter, the learning rate and the per-update scalars of the AdamW step in one small
 * device record, so that an update can be captured in a graph and replayed: nothing the update
 * depends on is baked into a launch.  Per update: trlx_adamw_advance (k_adamw_advance, one wave),
 * then the _dev step entries, which read the record where trlx_adamw_step reads its arguments.
 * trlx_adamw_advance, in this order:
 *   1. skip_nonfinite != 0, grad_record given and its `nonfinite` set: apply = 0, sync = 0,
 *      skipped += 1; step, lr and the scalars stay as they are; done.
 *   2. step += 1, apply = 1, lr = lr_table[min(step, n_lr) - 1] (entry k-1 is the rate of update
 *      k, the last entry holds afterwards).
 *   3. the nine scalars from step and lr as trlx_adamw_step forms them — in fp64, each rounded to
 *      fp32 once — with one difference: b^step is a square-and-multiply product chain over the
 *      bits of step (r = 1; for each bit from the lowest: if set r = r*x; x = x*x), every product
 *      a separately rounded fp64 multiplication, where trlx_adamw_step calls pow().  A CPU can
 *      restate a product chain bit for bit, not another library's pow; 1 - b^step, the division
 *      and the square root are IEEE-exact on both sides.  trlx_adamw_sched_scalars_host is the
 *      same function on the host (no device, no stream): out[9] = {decay, w1, b2, w2, neg_step,
 *      sqrt_bc2, eps, alpha, beta}.
 *   4. sync = (sync_every > 0 && step % sync_every == 0).
 * trlx_adamw_step_dev / trlx_adamw_step_clipped_dev are trlx_adamw_step / trlx_adamw_step_clipped
 * with the scalars read from `sched` on the device: step, lr, beta1, beta2, eps, weight_decay
 * and alpha of `args` are IGNORED (and not validated).  lr_table / n_lr of `args` name the table
 * the record's advance reads, so that the step can refuse a table its tensors would overwrite;
 * trlx_adamw_step and trlx_adamw_step_clipped never read the two fields.  With apply == 0 every workgroup returns
 * before its first load: nothing of p, m, v, master, target is read or written.  With sync == 0
 * the update is applied and `target` is neither read nor written.  For the same scalars the
 * result bits are those of trlx_adamw_step / trlx_adamw_step_clipped.
 * Refused before anything is launched (TRLX_ERR_ARG): a NULL sched or lr_table, a sched, lr_table
 * or grad_record not aligned to 8 bytes, n_lr < 1, sync_every < 0, a NaN hyper-parameter, any
 * overlap among sched, lr_table and grad_record (advance), a sched or an lr_table that overlaps
 * any tensor of the step, the clip record or each other, an lr_table not aligned to 8 bytes or
 * given with n_lr < 1 (_dev entries). */
typedef struct {
    int64_t step;                     /* updates applied so far */
    int64_t skipped;                  /* updates skipped because of a non-finite norm */
    int32_t apply;                    /* 1: the current update is applied */
    int32_t sync;                     /* 1: the current update syncs the targets */
    float decay, w1, b2, w2, neg_step, sqrt_bc2, eps;  /* 1 - lr*wd, 1-b1, b2, 1-b2, -(lr/bc1), sqrt(bc2), eps */
    float alpha, beta;                /* alpha and 1 - alpha of the folded sync */
    float pad;
    double lr;                        /* the rate of the current update, for inspection */
    int64_t reserved[3];
} trlx_adamw_sched;                   /* 96 bytes, 8-byte aligned */
typedef struct {
    void* sched;                      /* trlx_adamw_sched on the device, in/out */
    double beta1, beta2, eps, weight_decay;
    double alpha;                     /* of the folded sync */
    const void* lr_table;             /* device fp64 [n_lr] */
    int64_t n_lr;                     /* >= 1 */
    int64_t sync_every;               /* >= 0; 0: never */
    const void* grad_record;          /* NULL, or the trlx_grad_norm_record of this update */
    int skip_nonfinite;
} trlx_adamw_advance_args;
int trlx_adamw_advance(const trlx_adamw_advance_args* args, void* stream);
int trlx_adamw_sched_scalars_host(int64_t step, double lr, double beta1, double beta2, double eps,
                                  double weight_decay, double alpha, float* out);
int trlx_adamw_step_dev(const trlx_adamw_args* args, const void* sched, void* stream);
int trlx_adamw_step_clipped_dev(const trlx_adamw_args* args, const void* grad_record, const void* sched,
                                void* stream);

/* ---------------------------------------------------------------- AdamW with a bf16 state
 * trlx_adamw_step_ex is every launch form above behind one entry, with the dtype of m and v
 * chosen by the caller: grad_record NULL = unclipped (else as trlx_adamw_step_clipped), sched
 * NULL = the scalars of `args` (else as the _dev entries).  trlx_adamw_args is unchanged.
 * state_dtype = TRLX_F32: bit for bit trlx_adamw_step / _clipped / _dev / _clipped_dev.
 * state_dtype = TRLX_BF16: m and v are bf16 arrays — what torch.optim.AdamW keeps for a bf16
 * parameter (state = zeros_like(p)), the optimizer the reference trains its bf16 models with.
 * p and g are bf16 too and there is no master.  Per element, the same fp32 scalars, every op a
 * separately rounded fp32 op (no fma) whose result is rounded to bf16 (round-to-nearest-even)
 * wherever torch's _single_tensor_adam writes a bf16 tensor, bf(x) below:
 *   p = bf(p * (1 - lr*wd))                                              mul_
 *   m = bf(m + (1-b1) * (g - m))                                         lerp_
 *   v = bf(v * b2);  v = bf(v + (1-b2) * (g * g))                        mul_, addcmul_
 *   d = bf(sqrt(v));  d = bf(d / sqrt(bc2));  d = bf(d + eps)            sqrt, div, add_
 *   p = bf(p + (-(lr/bc1)) * (m / d))                                    addcdiv_
 * The products and the quotient inside lerp_, addcmul_ and addcdiv_ stay fp32.  With a clip
 * record g is first bf(g * bf(coef)), as in trlx_adamw_step_clipped with a bf16 g; a target is
 * updated from the stored p exactly as trlx_polyak_update's bf16 form does.  A bf16 v stops
 * moving once (1-b2) * g*g falls below half an ulp of v — torch's bf16 AdamW does the same.
 * All four arrays are 2-byte: one 16-byte vector per array per group of 8 elements wherever
 * p, g, m, v (and target) share a 16-byte phase, element accesses otherwise, same result bits.
 * HBM traffic per parameter: 14 B (read p, g, m, v, write p, m, v), 16 B clipped (the norm
 * reads g once more), 18 B with a target (+ read and write of the target); the fp32-state step
 * on bf16 p and g moves 22 B.
 * Refused before anything is launched: a state_dtype other than TRLX_F32 / TRLX_BF16, or
 * TRLX_BF16 with a p_dtype or g_dtype that is not TRLX_BF16 (TRLX_ERR_DTYPE); TRLX_BF16 with a
 * non-NULL master in a live entry, m or v not aligned to 2 bytes, a record or sched not aligned
 * to 8 bytes (TRLX_ERR_ARG); and everything the four entries above refuse, the overlap checks
 * taking m and v at their 2-byte extents. */
int trlx_adamw_step_ex(const trlx_adamw_args* args, int state_dtype, const void* grad_record, const void* sched,
                       void* stream);

/* ---------------------------------------------------------------- fused bf16 value head
 * The PPO value head — replaces `make_head(n_embd, 1)` (ppo_models.py:216-222: Linear(H, 2H),
 * ReLU, Linear(2H, 1), all bf16) and its use at :618,:641:
 *   z[t, j]   = bf16(sum_k h[t, k] * w1[j, k] + b1[j])      fp32 accumulation, ONE bf16 rounding
 *   values[t] = sum_j relu(z[t, j]) * w2[j] + b2            fp32 accumulation, rounded once
 * h: bf16 [N, H], row t at h + t*ldh (ldh >= H, a multiple of 8, <= 2^24; 16-byte aligned base);
 * w1: bf16 [2H, H] contiguous, 16-byte aligned; b1, w2: bf16 [2H]; b2: bf16 [1]; values: [N] of
 * values_dtype (TRLX_F32 / TRLX_BF16).  32 <= H <= 8192, H a multiple of 32, 1 <= N <= 2^30;
 * anything else is refused before any launch.  z is never written.  A workgroup owns 64 tokens
 * and one of S contiguous column slices; S = trlx_value_head_splits(N, H) is a function of N, H
 * and the device's compute units (tuning "vhead_splits" overrides it).  S = 1: one launch.
 * S > 1: one fp32 partial per (split, token) in `workspace`
 * (>= trlx_value_head_workspace_bytes(N, H), enough for every S; may be NULL when S = 1) and a
 * second small launch that adds them in split order.  For fixed (N, H, S) the result is
 * bit-reproducible and independent of ldh and of the base address. */
int trlx_value_head_splits(int64_t N, int64_t H);          /* 0 for a refused shape */
int64_t trlx_value_head_workspace_bytes(int64_t N, int64_t H);
int trlx_value_head_fwd(const void* h, int64_t ldh, const void* w1, const void* b1, const void* w2,
                        const void* b2, int64_t N, int64_t H, void* values, int values_dtype,
                        void* workspace, void* stream);

/* The head's own backward from dv [N] (dv_dtype TRLX_F32 / TRLX_BF16): z is recomputed and
 *   dz[t, j] = bf16(dv[t] * w2[j]) where z[t, j] > 0, else 0        bf16 [N, 2H], contiguous
 *   dw2[j]   = sum_t dv[t] * relu(z[t, j])      db1[j] = sum_t dz[t, j]      db2 = sum_t dv[t]
 * dw2, db1 [2H] and db2 [1] of grad_dtype, summed in fp32 in a fixed order (per 32-token half
 * block, then the half blocks in order) in `workspace`
 * (>= trlx_value_head_bwd_workspace_bytes(N, H)).  dh = dz * w1 and dw1 = dz^T * h are plain
 * GEMMs left to the caller's BLAS.  Two launches; operands and limits as the forward. */
int64_t trlx_value_head_bwd_workspace_bytes(int64_t N, int64_t H);
int trlx_value_head_bwd(const void* h, int64_t ldh, const void* w1, const void* b1, const void* w2,
                        const void* dv, int dv_dtype, int64_t N, int64_t H, void* dz, void* dw2,
                        void* db1, void* db2, int grad_dtype, void* workspace, void* stream);

/* ---------------------------------------------------------------- §8f rank 2: fused lm_head + logprobs
 * lp[n] = h[n]·W[y_n] − logsumexp_v h[n]·W[v] without materialising the [N, V] logits —
 * replaces `logits = lm_head(hs)` (ppo_models.py:640 T5HeadWithValueModel, :274/:588 GPT)
 * + logprobs_from_logits (modeling.py:37-41) on the experience side
 * (ppo_orchestrator.py:135-155, no gradient).  hidden: bf16 [N, H] rows of ldh elements;
 * weight: bf16 [V, H] (nn.Linear layout) rows of ldw; H a multiple of 64, rows 16-B
 * aligned.  labels int64 (stride lb; out of range -> NaN).  lp_out [N] of lp_dtype
 * (F32/BF16), lse_out optional fp32 [N].  MFMA (bf16 in, fp32 accumulate) tiles of
 * 256 tokens x 256 vocab (128 x 128 for small N) with an online max/Σexp epilogue, then a
 * per-token combine.
 * workspace: trlx_lmhead_workspace_bytes(N, V) bytes (no initialisation needed). */
int64_t trlx_lmhead_workspace_bytes(int64_t N, int64_t V);
/* Kernel variant (0 = automatic: 8 for N >= 2048, else 3; 3 = 128x128 tiles, 2 barriers per
 * K-step; 8 = 256x256 ping-pong, two wave groups staggered by a barrier, 2 phases per K-step).
 * Other values are rejected (the round-1 variants that measured slower were removed).  Results
 * identical up to fp32 summation order.  Set before sizing the workspace (the vocab tile width
 * changes it). */
int trlx_lmhead_set_variant(int variant);
int trlx_lmhead_logprobs(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                         int64_t H, int64_t V, const int64_t* labels, int64_t lb, void* lp_out,
                         int lp_dtype, float* lse_out, void* workspace, void* stream);
/* The same over a ragged batch: N = B·T tokens in rollouts of T, decoder lengths [B] int64.
 * Tokens past their rollout's length are store padding: lp (and lse) 0 there.  With an order
 * scratch (trlx_ragged_order_bytes(B, T) bytes) the 128 x 256 MFMA tiles (the H <= 1024,
 * N >= 2048 variant) gather the valid tokens' hidden rows and skip the padding's tiles — the
 * GEMM work of a batch of decoder lengths L_b is that of its sum(L_b) tokens; the other
 * variants compute every token and zero the padding's lp.  N·ldh·2 must stay below 2 GB. */
int trlx_lmhead_logprobs_ragged(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                                int64_t H, int64_t V, const int64_t* labels, int64_t lb, const int64_t* lengths,
                                int64_t T, void* order_ws, void* lp_out, int lp_dtype, float* lse_out,
                                void* workspace, void* stream);

/* ---------------------------------------------------------------- §8f rank 2, loss side: fused lm_head fwd + bwd
 * The policy update's lm_head (ppo_models.py:640 T5, :274 GPT) + logprobs_from_logits
 * (modeling.py:37-41) + autograd back through both (accelerate_ppo_model.py:96-118), with the
 * [N, V] logits and dlogits never written: with p = softmax(h·Wᵀ) and g = d loss / d lp,
 *   dh_t = g_t·(W[y_t] − Σ_v p_tv·W_v)      dW_v = Σ_t g_t·(1[y_t = v] − p_tv)·h_t.
 * hidden [N, ldh] bf16 (N = B·T tokens, row t of rollout b = token b·T + t), weight [V, ldw]
 * bf16 (nn.Linear layout), H in {512, 768}; dweight [V, lddw] of dw_dtype (overwritten); dhidden
 * [N, lddh] of dh_dtype (bf16 / fp32, lddh a multiple of 4).  Three MFMA launches + small
 * ones: a flash-style forward (online softmax and O = Σ_v P·W_v per token and vocab split), a
 * per-token combine (lse, lp, g, dh) and a dW pass that recomputes each logits tile and
 * accumulates dSᵀ·h — or, in the PPO entries given the larger saved-P workspace, reads the
 * forward's bf16 P tiles back instead of recomputing them; deterministic (fixed-order sums, no
 * atomics).
 * lm_workspace: trlx_lmhead_loss_workspace_bytes(N, H, V) bytes, no initialisation. */
int64_t trlx_lmhead_loss_workspace_bytes(int64_t N, int64_t H, int64_t V);
/* The PPO entries' workspace with room for the saved-P plan (the forward's bf16 P tiles,
 * ⌈V/64⌉·2⌈N/64⌉·4 KB: 0.62 GB at N = 6144, V = 50257, plus per-(split, token) records).  Pass
 * its size as lm_workspace_bytes; a workspace of only trlx_lmhead_loss_workspace_bytes runs the
 * recompute plan. */
int64_t trlx_ppo_loss_from_hidden_workspace_bytes(int64_t N, int64_t H, int64_t V);
/* The plan the PPO entries run for this shape and workspace size: 1 = saved P (three MFMA
 * passes: S and O forward, dSᵀ·h from the stored P), 0 = recompute (four: S recomputed in dW). */
int trlx_ppo_loss_from_hidden_plan(int64_t N, int64_t H, int64_t V, int64_t lm_workspace_bytes);
/* The smaller workspace trlx_lmhead_logprobs_bwd / _bwd_savep need (no forward partials). */
int64_t trlx_lmhead_loss_bwd_workspace_bytes(int64_t N, int64_t H, int64_t V);
/* The PPO loss from the policy's last hidden states: trlx_ppo_loss_rows's arguments with the
 * logits replaced by (hidden, weight) and dlogits by (dhidden, dweight) — same token records
 * in `workspace` (trlx_ppo_rollout_loss then emits loss + stats), same whitening of adv_raw by
 * `stats` (NULL: adv_raw used as given, and then only mask = NULL: the loss normaliser Σ mask
 * is read at stats[3]), dvalues, lp_out.  Tokens with mask == 0 are skipped (compacted out of
 * all three MFMA passes: zero gradient, lp_out 0, their token records as the masked loss rows
 * write them).  N·ldh·2 and V·ldw·2 must stay below 2 GB (32-bit tile addressing).
 * lm_workspace_bytes: the size of lm_workspace (>= trlx_lmhead_loss_workspace_bytes, else
 * TRLX_ERR_ARG; >= trlx_ppo_loss_from_hidden_workspace_bytes selects the saved-P plan). */
int trlx_ppo_loss_from_hidden(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t B,
                              int64_t T, int64_t H, int64_t V, const int64_t* labels, const void* old_lp,
                              int old_dtype, const float* adv_raw, const double* stats, int unbiased,
                              const int64_t* mask, const void* values, int v_dtype, const void* old_values,
                              int ov_dtype, const void* returns, int r_dtype, float cliprange,
                              float cliprange_value, float vf_coef, float* lp_out, void* dhidden, int64_t lddh,
                              int dh_dtype, void* dweight, int dw_dtype, int64_t lddw, float* dvalues,
                              void* workspace, void* lm_workspace, int64_t lm_workspace_bytes, void* stream);
/* The split-beta form (the pipelined data-parallel schedule; see trlx_ppo_loss_rows_split /
 * trlx_ppo_loss_rows_split_gae): the advantage A0 - beta*Ak whitened by coefficients that are
 * either given (`coef`, stored by an earlier loss on the same experience) or derived here from
 * the all-reduced split record `stats8` and beta (ctl_state[TRLX_CTL_KL_COEF], or kl_coef when
 * ctl_state is NULL; `unbiased` as there) and stored to coef_out (may be NULL) — exactly one of
 * coef / stats8.  The batch's rewards and returns (r_dtype) are written here; msum = Σ mask
 * (stats8 + 6; required with a mask); the loss tail takes stats8 + 3 as its `stats`. */
int trlx_ppo_loss_from_hidden_split(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t B,
                                    int64_t T, int64_t H, int64_t V, const int64_t* labels, const void* old_lp,
                                    int old_dtype, const float* adv0, const float* adv_kl, const float* rew_kl,
                                    const float* rew_score, const float* coef, const double* stats8, int unbiased,
                                    const double* ctl_state, float kl_coef, float* coef_out, const double* msum,
                                    const int64_t* mask, const void* values, int v_dtype, const void* old_values,
                                    int ov_dtype, float* rewards, void* returns, int r_dtype, float cliprange,
                                    float cliprange_value, float vf_coef, float* lp_out, void* dhidden, int64_t lddh,
                                    int dh_dtype, void* dweight, int dw_dtype, int64_t lddw, float* dvalues,
                                    void* workspace, void* lm_workspace, int64_t lm_workspace_bytes,
                                    void* stream);
/* The differentiable building block (logprobs_from_logits(lm_head(h), y) with autograd):
 * forward -> lp [N] (lp_dtype), lse [N] fp32 and E = Σ_v p_tv·W_v [N, H] fp32 (saved for the
 * backward); backward(grad = d loss / d lp [N], F32 / BF16) -> dhidden, dweight (either may be
 * NULL: a frozen lm_head skips the dW pass; lm_workspace: trlx_lmhead_loss_bwd_workspace_bytes). */
int trlx_lmhead_logprobs_fwd_saved(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                                   int64_t H, int64_t V, const int64_t* labels, int64_t lb, void* lp_out,
                                   int lp_dtype, float* lse_out, float* e_out, void* lm_workspace, void* stream);
int trlx_lmhead_logprobs_bwd(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                             int64_t H, int64_t V, const int64_t* labels, int64_t lb, const void* grad,
                             int grad_dtype, const float* lse, const float* e, void* dhidden, int64_t lddh,
                             int dh_dtype, void* dweight, int dw_dtype, int64_t lddw, void* lm_workspace,
                             void* stream);
/* The same pair, extended (replaces the same reference lines as the pair above:
 * accelerate_ppo_model.py:96-118 through ppo_models.py:640 and modeling.py:37-41):
 *   saved: NULL = the recompute plan (as above), or a region of trlx_lmhead_savep_bytes(N, H, V)
 *          bytes (2⌈V/128⌉·2⌈N/64⌉·4 KB + 32·N B: 0.62 GB at N = 6144, V = 50257 — the size of
 *          bf16 logits) the forward fills with its bf16 P tiles and per-(split, token) records
 *          and the caller keeps, unmodified, until the backward: the dW pass then reads P back
 *          (3 MFMA passes in all) instead of recomputing S (4);
 *   mask:  NULL = every token, or [N] int64: tokens with mask == 0 are compacted out of every
 *          MFMA pass — their lp and lse are 0 and they get a zero dh and no share of dW (what the
 *          PPO loss's own mask gives them: ppo_models.py:150-199 multiplies every lp term by it).
 *          The backward takes the same mask (it rebuilds the same stable order).
 * The forward-to-backward plan contract: the saved P tiles and records are laid out by the
 * forward's split plan ("lmloss_splits": fixed count or auto) and split granule, and the
 * backward must map them the same way.  The *_ex2 pair carries that plan itself: the forward
 * writes a host-side token to *plan_out (the "lmloss_splits", "lmloss_dwp_form" and "lmloss_dw"
 * values it read, once), the backward takes it by value and reads none of those knobs, so the
 * tuning may change between the two calls (a backward with a token of a forward that kept P
 * runs the saved-P dW pass in the forward's form; a value that is no token: TRLX_ERR_ARG).
 * The *_ex pair has no token: its backward reads the knobs again, and the caller must hold
 * those three unchanged from the forward to the backward.  lm_workspace as the pair above. */
int64_t trlx_lmhead_savep_bytes(int64_t N, int64_t H, int64_t V);
int trlx_lmhead_logprobs_fwd_ex(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                                int64_t H, int64_t V, const int64_t* labels, int64_t lb, const int64_t* mask,
                                void* lp_out, int lp_dtype, float* lse_out, float* e_out, void* lm_workspace,
                                void* saved, void* stream);
int trlx_lmhead_logprobs_bwd_ex(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                                int64_t H, int64_t V, const int64_t* labels, int64_t lb, const int64_t* mask,
                                const void* grad, int grad_dtype, const float* lse, const float* e, void* dhidden,
                                int64_t lddh, int dh_dtype, void* dweight, int dw_dtype, int64_t lddw,
                                void* lm_workspace, const void* saved, void* stream);
int trlx_lmhead_logprobs_fwd_ex2(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                                 int64_t H, int64_t V, const int64_t* labels, int64_t lb, const int64_t* mask,
                                 void* lp_out, int lp_dtype, float* lse_out, float* e_out, void* lm_workspace,
                                 void* saved, int64_t* plan_out, void* stream);
int trlx_lmhead_logprobs_bwd_ex2(const void* hidden, int64_t ldh, const void* weight, int64_t ldw, int64_t N,
                                 int64_t H, int64_t V, const int64_t* labels, int64_t lb, const int64_t* mask,
                                 const void* grad, int grad_dtype, const float* lse, const float* e, void* dhidden,
                                 int64_t lddh, int dh_dtype, void* dweight, int dw_dtype, int64_t lddw,
                                 void* lm_workspace, const void* saved, int64_t plan, void* stream);

/* ---------------------------------------------------------------- §8f rank 3: ILQL sampling step
 * One decode step of CausalLMWithValueHeads.generate (ilql_models.py:296-316) per row b:
 *   score = log_softmax(logits[b]) + beta*(min(tq0[b], tq1[b]) - vs[b])  (logits -inf where
 *   logit_mask[prev_ids[b]] is set), topk_mask(score, top_k) (:24-28, ties at the threshold
 *   kept), pi = softmax(. / temperature); out_ids[b] = the inverse CDF of pi at u[b] (index
 *   order; u from the caller's generator replaces torch.multinomial's draw);
 *   out = finished ? eos : out; finished = out == eos.
 * logits / tq rows: [B, V] of dtype with row strides ld_*; tq1 may be NULL (one head);
 * logit_mask: NULL or uint8 [*, V] rows of ld_mask; finished: int64 [B] in/out or NULL.
 * A row in which nothing is kept (no finite logit) returns token 0.  B == 0 launches nothing
 * (the row pointers may then be NULL). */
int trlx_ilql_sample(const void* logits, int64_t ld_logits, const void* tq0, int64_t ld_tq0,
                     const void* tq1, int64_t ld_tq1, int dtype, const float* vs,
                     const uint8_t* logit_mask, int64_t ld_mask, const int64_t* prev_ids, int64_t B,
                     int64_t V, float beta, int top_k, float temperature, const float* u,
                     int64_t* out_ids, int64_t* finished, int64_t eos, void* stream);

/* ---------------------------------------------------------------- PPO rollout sampling step
 * One decode step of HF generate's sample path (transformers 4.21; ppo_orchestrator.py:76 with
 * PPOConfig.gen_kwargs) per row b, x = logits[b] in fp32:
 *   x[eos] = -inf while cur_len < min_length (eos given);
 *   top-k: keep x >= the k-th largest x, k = min(max(top_k, min_tokens_to_keep), V), ties at
 *   the threshold kept, top_k = 0 off;
 *   top-p (only when top_p < 1): w = exp((x - max x) / temperature) over the top-k survivors,
 *   W = sum w; x is kept iff the mass of the survivors strictly above it is <= top_p * W (the
 *   token that crosses top_p stays) or it is among the min_tokens_to_keep largest; every tie
 *   at the nucleus boundary is kept (HF keeps the one its sort placed first);
 *   out_ids[b] = the inverse CDF of w over the kept at u[b], vocab-index order (u from the
 *   caller's generator replaces torch.multinomial's draw);
 *   unfinished[b] == 0: out_ids[b] = pad and the row does no other work; else
 *   unfinished[b] &= out_ids[b] != eos.
 * out_logprobs[b] = log_softmax(logits[b])[out_ids[b]] on the unmodified row (no eos
 * suppression, no temperature); out_min_kept[b] = the smallest kept x, exactly;
 * out_kept_count[b] = the number of kept tokens.  A finished row writes 0 to those three; so
 * does a row with no finite logit left, which returns pad (HF raises there); pad = -1 writes
 * token 0 in both cases.  The row without a finite logit updates unfinished[b] like any live
 * row, from the token it returns: a pad that equals eos finishes it (HF: a sequence ends at
 * eos), any other pad leaves it live; eos = -1 leaves unfinished untouched for every row.
 * logits: [B, V] of dtype (TRLX_F32 / TRLX_BF16), row stride ld_logits, unit column stride;
 * eos_token_id / pad_token_id in [0, V) or -1 for none; unfinished: int64 [B] in/out or NULL.
 * Requires temperature > 0, top_p > 0, top_k >= 0, min_tokens_to_keep >= 1 (TRLX_ERR_ARG);
 * B = 0 is a no-op.  Stream-ordered: no host synchronisation, no allocation. */
int trlx_ppo_sample(const void* logits, int64_t ld_logits, int dtype, int64_t B, int64_t V,
                    float temperature, int top_k, float top_p, int min_tokens_to_keep,
                    int64_t cur_len, int64_t min_length, int64_t eos_token_id, int64_t pad_token_id,
                    const float* u, int64_t* out_ids, float* out_logprobs, float* out_min_kept,
                    int32_t* out_kept_count, int64_t* unfinished, void* stream);

/* The recording step: trlx_ppo_sample (the same arguments, the same policy-row path: token,
 * out_logprobs, out_min_kept and out_kept_count are bit-identical) that also scores the token
 * under the reference model's row of the same step and writes column t of the rollout's
 * [B, T] buffers, so no teacher-forced second pass over [B, T, V] logits is needed
 * (ppo_orchestrator.py:116-161):
 *   ref_logits: [B, V] rows of ref_dtype (must equal dtype), row stride ld_ref, streamed once
 *   and reduced to (max, sum exp) in fp32 in a fixed order;
 *   tokens[b, t] = out_ids[b];  logprobs[b, t] = out_logprobs[b];
 *   ref_logprobs[b, t] = log_softmax(ref_logits[b])[out_ids[b]];
 *   values[b, t] = step_values[b] (values_dtype TRLX_F32 / TRLX_BF16; both NULL = none);
 *   lengths[b] = t + 1 where a live row returns eos (NULL = not kept; a row that stays live
 *   leaves its entry untouched: the caller initialises lengths to T).
 * Finished rows (unfinished[b] == 0): score_finished = 0 writes pad, 0, 0 and value 0 and reads
 * neither row (the ragged convention of the experience kernels); score_finished = 1 writes pad
 * and the log-softmax of both rows at pad (also to out_logprobs[b]) and the value as given —
 * what a teacher-forced pass with an all-ones mask stores after eos — with no selection and no
 * draw; the row stays finished either way.  A live row with no finite policy logit records pad, 0, 0.
 * Record buffers: row strides in elements, each >= T; 0 <= t < T.  Launch table and vocab
 * limit as trlx_ppo_sample. */
int trlx_ppo_sample_record(const void* logits, int64_t ld_logits, int dtype, int64_t B, int64_t V,
                           float temperature, int top_k, float top_p, int min_tokens_to_keep,
                           int64_t cur_len, int64_t min_length, int64_t eos_token_id, int64_t pad_token_id,
                           const float* u, int64_t* out_ids, float* out_logprobs, float* out_min_kept,
                           int32_t* out_kept_count, int64_t* unfinished, const void* ref_logits,
                           int64_t ld_ref, int ref_dtype, int64_t t, int64_t T, int64_t* tokens,
                           int64_t ld_tokens, float* logprobs, int64_t ld_logprobs, float* ref_logprobs,
                           int64_t ld_ref_logprobs, float* values, int64_t ld_values,
                           const void* step_values, int values_dtype, int64_t* lengths,
                           int score_finished, void* stream);

/* The processing step: trlx_ppo_sample / trlx_ppo_sample_record with HF's prefix-aware logits
 * processors and the forced token (transformers 4.21 _get_logits_processor order; the rollouts
 * of T5HeadWithValueModel.generate, ppo_models.py:620-622, pass forced_bos_token_id and any
 * gen_kwargs key).  The prefix of row b — HF's input_ids[b], the same length n = prefix0_len +
 * prefix1_len for every row, pad tokens counted like any other — is prefix0[b, 0:prefix0_len]
 * followed by prefix1[b, 0:prefix1_len] (device int64, row strides in elements).  The processed
 * row of a live row, x = logits[b] in fp32:
 *   1. repetition_penalty rp != 1: for every distinct prefix token v,
 *      x[v] = x[v] < 0 ? x[v] * rp : x[v] / rp (fp32 multiplication / division, correctly
 *      rounded: equal to torch's on fp32 rows; bf16 rows are not rounded back to bf16);
 *   2. no_repeat_ngram_size g > 0, when n + 1 >= g: for every i with
 *      p[i : i+g-1] == p[n-g+1 : n], x[p[i+g-1]] = -inf (g = 1 bans every prefix token);
 *   3. bad words, n_bad_words sequences s = bad_words[off[s] .. off[s+1]) = [w0 .. wk]:
 *      k = 0 always gives x[w0] = -inf; k >= 1 bans wk when n >= k and the prefix ends
 *      with w0 .. w(k-1);
 *   4. x[eos] = -inf while cur_len < min_length, as trlx_ppo_sample;
 *   5. forced_token_id f >= 0 (the caller's forced bos / eos decision for this cur_len): every
 *      entry -inf except x[f] = 0 — out_ids[b] = f, out_min_kept[b] = 0, out_kept_count[b] = 1;
 *   6. temperature, top-k, top-p, the draw at u[b], unfinished / pad, as trlx_ppo_sample.
 * out_logprobs, and with a record block logprobs[b, t] and ref_logprobs[b, t], stay the
 * log-softmax of the unmodified rows at the token, forced tokens included; out_min_kept and
 * out_kept_count describe the processed row.  A prefix token outside [0, V) is ignored by every
 * processor (tested before any address is formed); it keeps its position in the n-gram and
 * bad-word matches, which compare the int64 values.  Finished rows as in the other two entries.
 * Record block: ref_logits == NULL is the plain step and the block is not read; otherwise its
 * fields and checks are trlx_ppo_sample_record's.
 * Bad words: the device table (bad_words, bad_words_offsets of n_bad_words + 1 entries) is
 * what the kernel reads; bad_words_host / bad_words_offsets_host are the same arrays in host
 * memory, read during the call only, and are what the argument checks read.
 * Refused before any launch: repetition_penalty <= 0, no_repeat_ngram_size < 0, forced_token_id
 * outside [-1, V), a bad-word token outside [0, V), offsets that do not start at 0 or do not
 * ascend strictly, a missing table pointer (TRLX_ERR_ARG); a segment with n > 0 and a NULL
 * pointer (TRLX_ERR_ARG) or a row stride below n (TRLX_ERR_SHAPE); and whatever the other two
 * entries refuse.  With repetition_penalty = 1, no_repeat_ngram_size = 0, n_bad_words = 0 and
 * forced_token_id = -1 the call launches the kernel of trlx_ppo_sample / trlx_ppo_sample_record. */
typedef struct TrlxPpoSampleProcArgs {
    /* the plain step: the arguments of trlx_ppo_sample */
    const void* logits;
    int64_t ld_logits;
    int64_t B;
    int64_t V;
    int dtype;
    int top_k;
    float temperature;
    float top_p;
    int min_tokens_to_keep;
    int score_finished;
    int64_t cur_len;
    int64_t min_length;
    int64_t eos_token_id;
    int64_t pad_token_id;
    const float* u;
    int64_t* out_ids;
    float* out_logprobs;
    float* out_min_kept;
    int32_t* out_kept_count;
    int64_t* unfinished;
    /* the record block: the arguments of trlx_ppo_sample_record (score_finished above) */
    const void* ref_logits;
    int64_t ld_ref;
    int64_t t;
    int64_t T;
    int64_t* tokens;
    int64_t ld_tokens;
    float* logprobs;
    int64_t ld_logprobs;
    float* ref_logprobs;
    int64_t ld_ref_logprobs;
    float* values;
    int64_t ld_values;
    const void* step_values;
    int64_t* lengths;
    int ref_dtype;
    int values_dtype;
    /* the processor block */
    float repetition_penalty;
    int no_repeat_ngram_size;
    int64_t forced_token_id;
    const int64_t* prefix0;
    int64_t prefix0_ld;
    int64_t prefix0_len;
    const int64_t* prefix1;
    int64_t prefix1_ld;
    int64_t prefix1_len;
    const int64_t* bad_words;
    const int64_t* bad_words_offsets;
    const int64_t* bad_words_host;
    const int64_t* bad_words_offsets_host;
    int64_t n_bad_words;
} TrlxPpoSampleProcArgs;
int trlx_ppo_sample_proc(const TrlxPpoSampleProcArgs* a, void* stream);

/* The recording / processing step with its per-token scalars read from the decode clock (the
 * record documented at trlx_decode_clock_init below): the same launch arguments at every token.
 * The record block is required (a->ref_logits != NULL).  a->t, a->cur_len, a->forced_token_id and
 * a->prefix1_len are not read; the kernel derives, from the clock's t and cur_len0:
 *   t            the record column
 *   cur_len      cur_len0 + t;  eos is suppressed while eos >= 0 && cur_len < min_length
 *   forced token forced_eos_token_id at cur_len == max_length - 1, else forced_bos_token_id at
 *                cur_len == 1, else none (eos wins when both fire)
 *   prefix1_len  t; prefix1 / prefix1_ld are a->prefix1 / a->prefix1_ld when a->prefix1 is given
 *                (row stride >= T - 1), else the record's own tokens / ld_tokens
 *   u            u_ld == 0: u[b]; u_ld >= B: u[t * u_ld + b], row t of a [T, u_ld] table
 * a->T must equal the clock's T; the step is live iff 0 <= t < min(a->T, clock T).  A live step
 * is bit-identical, in every output and every record buffer, to trlx_ppo_sample_proc called with
 * those host values.  A dead step stores nothing: no output, no record column, no unfinished and
 * no lengths entry changes.  The processing kernel runs when a processor or either forced id is
 * set, otherwise the recording kernel; each in its device-clock instantiation, on the launch
 * table of trlx_ppo_sample.
 * Refused with TRLX_ERR_ARG before any launch: a NULL d or clock, a clock not aligned to 8 bytes,
 * u_ld not 0 and below B, a forced id outside [-1, V), forced_eos_token_id >= 0 with max_length
 * < 1, a missing record block; and everything trlx_ppo_sample_proc refuses (t is not checked). */
typedef struct TrlxPpoSampleDevArgs {
    const int64_t* clock;          /* the decode clock record */
    int64_t forced_bos_token_id;   /* -1 = none; forced at cur_len == 1 */
    int64_t forced_eos_token_id;   /* -1 = none; forced at cur_len == max_length - 1; wins over bos */
    int64_t max_length;            /* read only with forced_eos_token_id >= 0 */
    int64_t u_ld;                  /* 0: u is [B]; >= B: u is a [T, u_ld] table, row t is this step's */
} TrlxPpoSampleDevArgs;
int trlx_ppo_sample_proc_dev(const TrlxPpoSampleProcArgs* a, const TrlxPpoSampleDevArgs* d, void* stream);

/* ---------------------------------------------------------------- T5 decode-step attention
 * One query token per (batch row, head) over a device KV cache — replaces, per decoder layer
 * and generated token, the body of HF's T5Attention between the q / k / v projections and the
 * `o` projection (cache append, [B, nH, 1, t] matmul, compute_bias, mask add, fp32 softmax,
 * second matmul) with ONE launch, one workgroup per (batch row, head).  T5's attention: no
 * 1/sqrt(d) scaling, a bucketed relative-position bias added to the self-attention scores, an
 * encoder key mask on the cross-attention.  Forward only (generation runs under no_grad).
 *   q, k_new, v_new : [B, n_heads, d_kv] of `dtype` as a base pointer + a row stride in elements
 *                     (ldq, ldk, ldv >= n_heads * d_kv; head h at offset h * d_kv): a
 *                     [B, 1, n_heads * d_kv] projection output or a slice of a fused qkv
 *                     projection is read in place.  With B == 1 the strides are not read.
 *   out             : [B, n_heads * d_kv] of `dtype`, contiguous — what `o` takes.
 * mode TRLX_T5_ATTN_SELF, kv_len = t + 1:
 *   k, v : the cache [B, n_heads, max_len, d_kv], contiguous (HF's layout), in/out.  k_new[b, h, :]
 *   and v_new[b, h, :] are stored to column t; no other column is written, columns above t are
 *   never read, and key / value t are taken from the registers that hold k_new / v_new, never
 *   read back from the cache.
 *     score_j = q · k_j + bias_by_distance[h, t - j]          0 <= j <= t
 *   bias_by_distance: fp32 [n_heads, max_len] or NULL (no bias); key_mask must be NULL.
 * mode TRLX_T5_ATTN_CROSS, kv_len = max_len = S:
 *   k, v : [B, n_heads, S, d_kv], contiguous, read only; k_new, v_new, bias_by_distance NULL; t is
 *   not read.  key_mask: int64 [B, S] or NULL; a key with key_mask[b, j] == 0 is excluded from the
 *   softmax and neither its key nor its value row is read (holes allowed).
 *     score_j = q · k_j                                        key_mask[b, j] != 0
 * out[b, h, :] = sum_j softmax(score)_j * v_j.  The dot products, the bias add, the online
 * max / sum of the softmax and P·V are fp32; scores and probabilities are never rounded to
 * `dtype`; the result is rounded once.  A row whose keys are all masked gives zeros (HF's additive
 * finfo.min gives the plain average of the values there).  Fixed summation order: the result is
 * bit-reproducible and does not depend on B or on the strides.
 * Refused with TRLX_ERR_ARG before any launch: a dtype other than TRLX_F32 / TRLX_BF16, a d_kv
 * other than 64 / 128, a NULL q / k / v / out (self: k_new / v_new), t outside [0, max_len), a row
 * stride below n_heads * d_kv or not a whole number of 16-byte vectors, a q / k_new / v_new / k / v
 * / out that is not 16-byte aligned, a pointer of the other mode that is not NULL, B, n_heads or
 * max_len < 1. */
#define TRLX_T5_ATTN_SELF 0
#define TRLX_T5_ATTN_CROSS 1
typedef struct TrlxT5DecodeAttnArgs {
    const void* q;
    int64_t ldq;
    const void* k_new;                /* self only */
    int64_t ldk;
    const void* v_new;                /* self only */
    int64_t ldv;
    void* k;                          /* self: the cache, column t written; cross: read only */
    void* v;
    const float* bias_by_distance;    /* self only: [n_heads, max_len] fp32, or NULL */
    const int64_t* key_mask;          /* cross only: [B, S] int64, 0 = masked, or NULL */
    void* out;                        /* [B, n_heads * d_kv] */
    int64_t B;
    int64_t n_heads;
    int64_t d_kv;                     /* 64 or 128 */
    int64_t max_len;                  /* self: cache columns; cross: S */
    int64_t t;                        /* self: the column of the new token, kv_len = t + 1 */
    int dtype;                        /* TRLX_F32 / TRLX_BF16: q, k_new, v_new, k, v, out */
    int mode;                         /* TRLX_T5_ATTN_SELF / TRLX_T5_ATTN_CROSS */
} TrlxT5DecodeAttnArgs;
int trlx_t5_decode_attn(const TrlxT5DecodeAttnArgs* a, void* stream);

/* ---------------------------------------------------------------- the decode clock
 * The by-value scalars of a decode step that change every token — t of trlx_t5_decode_attn; t,
 * cur_len, forced_token_id and prefix1_len of trlx_ppo_sample_proc — as a device record, so that
 * the step's launches take the same arguments at every token and a graph captured once
 * (hipGraph, torch.cuda.graph) replays the whole rollout.  The record is eight int64 words
 * (64 bytes, 8-byte aligned, device memory):
 *   word 0  t         the next decode step, which is also the next column
 *   word 1  T         the capacity; a step issued with t outside [0, T) does nothing
 *   word 2  cur_len0  HF's cur_len at t = 0 (1 for T5: the decoder start token)
 *   word 3  overrun   the number of advances issued with t >= T; sticky
 *   word 4-7          reserved, zero
 * trlx_decode_clock_init sets {0, T, cur_len0, 0, 0, 0, 0, 0}; trlx_decode_clock_advance is one
 * one-thread launch: t < T ? t += 1 : overrun += 1.  Both are stream-ordered, synchronise nothing
 * and allocate nothing.  Nothing advances the clock implicitly: a decode step is the device-clock
 * entries below, in any order, followed by one trlx_decode_clock_advance.
 * Refused with TRLX_ERR_ARG before any launch: a NULL record or one not aligned to 8 bytes;
 * init: T < 1, cur_len0 < 0. */
#define TRLX_CLOCK_T 0
#define TRLX_CLOCK_CAP 1
#define TRLX_CLOCK_CUR_LEN0 2
#define TRLX_CLOCK_OVERRUN 3
#define TRLX_CLOCK_WORDS 8
int trlx_decode_clock_init(int64_t* clock, int64_t T, int64_t cur_len0, void* stream);
int trlx_decode_clock_advance(int64_t* clock, void* stream);

/* trlx_t5_decode_attn, mode TRLX_T5_ATTN_SELF, with t read from the clock (a->t is not read).
 * The step is live iff 0 <= t < min(clock T, max_len).  A live step is bit-identical to
 * trlx_t5_decode_attn called with that t: out, column t of both caches, nothing else written.
 * A dead step writes zeros to out and touches neither cache: every workgroup leaves before it
 * forms an address from t.  Every other field, check and refusal is trlx_t5_decode_attn's; also
 * refused with TRLX_ERR_ARG: a NULL clock, a clock not aligned to 8 bytes, mode
 * TRLX_T5_ATTN_CROSS (the cross step reads no t: trlx_t5_decode_attn is already the same launch
 * at every token). */
int trlx_t5_decode_attn_dev(const TrlxT5DecodeAttnArgs* a, const int64_t* clock, void* stream);

/* trlx_t5_decode_attn with a per-row skip: live is int64 [B], 0 or non-zero (the recording step's
 * `unfinished` is passed as it is).  clock: NULL for the host t (self) and for the cross mode, or
 * the decode clock for the self mode as in trlx_t5_decode_attn_dev (a->t is then not read).
 * A workgroup of a row with live[b] == 0 loads that one word, writes zeros to out[b, h, :] and
 * returns, before any barrier and before it forms an address into q, k_new, v_new, k, v, key_mask
 * or bias_by_distance; in the self mode column t of both caches stays unwritten for that row.  A
 * row with live[b] != 0 is bit-identical, in out and in column t of the caches, to
 * trlx_t5_decode_attn (host t, cross) / trlx_t5_decode_attn_dev (clock) with the same arguments.
 * Kernels of their own: the instantiations behind the two entries above are not touched.
 * For rollouts whose recording step runs with score_finished = 0: with score_finished != 0 the
 * sampler would score the pad of a row whose attention was skipped.  Within one decode step every
 * layer's call reads live before that step's sampling launch writes it (stream order).
 * Refused with TRLX_ERR_ARG before any launch: a NULL live, a live or clock not aligned to 8
 * bytes, a clock with mode TRLX_T5_ATTN_CROSS; and everything trlx_t5_decode_attn refuses (with a
 * clock, t is not checked). */
int trlx_t5_decode_attn_live(const TrlxT5DecodeAttnArgs* a, const int64_t* live, const int64_t* clock, void* stream);

/* ---------------------------------------------------------------- fp8 encoder keys and values
 * The encoder's projected keys and values are written once per rollout and read once per generated
 * token and layer.  trlx_t5_cross_kv_quantize stores them as OCP e4m3fn bytes with one
 * power-of-two scale per (batch row, head) and tensor; trlx_t5_decode_attn_kv8 is the cross step
 * over those bytes: half the K / V traffic, fp32 arithmetic.  Opt-in and lossy against the bf16
 * keys (e4m3 keeps 3 mantissa bits); exact against its own dequantised values (below).
 *
 * trlx_t5_cross_kv_quantize: ONE launch, K and V together, one workgroup per (b, h).
 *   k, v     : bf16 [B, n_heads, S, d_kv] as a base pointer + element strides over (b, h, s), unit
 *              stride along d_kv: a contiguous [B, nH, S, d] tensor (strides nH*S*d, S*d, d) and
 *              the projection output [B, S, nH*d] (strides S*nH*d, d, nH*d) are both read in
 *              place.  The stride of a dimension of size 1 is not read.
 *   key_mask : int64 [B, S], 0 = masked, or NULL.
 *   k8, v8   : bytes, contiguous [B, n_heads, S, d_kv].  k_scale, v_scale: fp32 [B, n_heads].
 * Per (b, h), separately for K and V:
 *   amax  = max |x| over the keys with key_mask != 0; a masked row is not read and is stored as
 *           zero bytes
 *   e     = the smallest integer with amax * 2^-e <= 448: with frexp(amax) = (m, x), x - 9 if
 *           m <= 0.875, else x - 8; 0 for amax == 0; then clamped to [-100, 119]
 *   scale = 2^e;  byte = e4m3fn(x * 2^-e), round to nearest, ties to even
 * x * 2^-e is exact in fp32, and the rounding restates torch's .to(torch.float8_e4m3fn) in integer
 * arithmetic, so the bytes are torch's cast of the scaled values bit for bit (torch's cast turns
 * what lies above 464 into the NaN byte; only an amax above 448 * 2^119, past the upper clamp,
 * gets there).  byte * scale is exactly representable in bf16: the attention below computes on values
 * that the bf16 entries can be fed bit for bit.
 * A live Inf or NaN in a (b, h) block of K (of V): that block's scale is NaN and each of its live
 * bytes is 0x7f, the e4m3fn NaN; the attention then gives NaN for that (b, h) and no other.
 * Refused with TRLX_ERR_ARG before any launch: NULL a / k / v / k8 / v8 / k_scale / v_scale, a
 * d_kv other than 64 / 128, B, n_heads or S < 1, k / v / k8 / v8 not 16-byte aligned, a scale not
 * 4-byte or key_mask not 8-byte aligned, a stride that is negative or not a whole number of
 * 16-byte vectors, a head or key stride below d_kv. */
typedef struct TrlxT5CrossKvQuantArgs {
    const void* k;                    /* bf16 */
    int64_t k_stride_b, k_stride_h, k_stride_s;
    const void* v;                    /* bf16 */
    int64_t v_stride_b, v_stride_h, v_stride_s;
    const int64_t* key_mask;          /* [B, S] int64, 0 = masked, or NULL */
    void* k8;                         /* [B, n_heads, S, d_kv] bytes */
    void* v8;
    float* k_scale;                   /* [B, n_heads] */
    float* v_scale;
    int64_t B;
    int64_t n_heads;
    int64_t S;
    int64_t d_kv;                     /* 64 or 128 */
} TrlxT5CrossKvQuantArgs;
int trlx_t5_cross_kv_quantize(const TrlxT5CrossKvQuantArgs* a, void* stream);

/* trlx_t5_decode_attn, mode TRLX_T5_ATTN_CROSS, over the quantiser's bytes: a->k and a->v are k8 and
 * v8, a->dtype is TRLX_BF16 (q and out), every other field as in the cross mode.
 *   score_j      = (q · k8_j) * k_scale[b, h]                  key_mask[b, j] != 0
 *   out[b, h, :] = (sum_j p_j * v8_j) * v_scale[b, h] / sum_j p_j,   p_j = exp(score_j - max)
 * The bytes are converted to fp32 in hardware; the dot, the online softmax and P·V are fp32, the
 * result is rounded once.  Masked keys are not read; a row whose keys are all masked gives zeros.
 * Fixed merge order: bit-reproducible, independent of B and of q's stride.
 * live: NULL, or int64 [B] with the semantics of trlx_t5_decode_attn_live: a workgroup of a row
 * with live[b] == 0 loads that one word, writes zeros to out[b, h, :] and returns before any
 * barrier and before it forms any other address.  The launch takes the same arguments at every
 * token: it captures as it is.
 * Refused with TRLX_ERR_ARG before any launch: everything the cross mode of trlx_t5_decode_attn
 * refuses (k and v not 16-byte aligned among it), mode TRLX_T5_ATTN_SELF, a dtype other than
 * TRLX_BF16, a NULL scale or one not 4-byte aligned, a live not 8-byte aligned. */
int trlx_t5_decode_attn_kv8(const TrlxT5DecodeAttnArgs* a, const float* k_scale, const float* v_scale,
                            const int64_t* live, void* stream);

/* ---------------------------------------------------------------- encoder keys shared by a prompt's samples
 * trlx_t5_decode_attn, mode TRLX_T5_ATTN_CROSS, for a rollout that draws G samples per prompt
 * (num_return_sequences, RLOO / GRPO groups, best-of-G): the encoder's keys and values are kept
 * once per prompt, [P, ...], and row b = p * G + g of q / out / live is sample g of prompt p — the
 * order of repeat_interleave(G, dim = 0).  ONE launch, one workgroup per (prompt, head, tile of
 * queries): each key and value row is loaded once and applied to every query of the tile, so the
 * K / V bytes per token and the K / V memory are those of trlx_t5_decode_attn divided by G.
 *   q, out   : [P * G, n_heads * d_kv] of `dtype`; q as a base pointer + row stride ldq as in
 *              trlx_t5_decode_attn (with P * G == 1 the stride is not read), out contiguous.
 *   k, v     : [P, n_heads, S, d_kv] of `dtype`, read only, as a base pointer + element strides
 *              over (p, h, s), unit stride along d_kv: a contiguous [P, nH, S, d] tensor (strides
 *              nH*S*d, S*d, d) and the projection output [P, S, nH*d] (strides S*nH*d, d, nH*d) are
 *              both read in place.  The stride of a dimension of size 1 is not read.
 *   key_mask : int64 [P, S], per prompt, 0 = masked, or NULL.  A masked key's K and V rows are not
 *              read; a prompt whose keys are all masked gives zeros in all its rows.
 *   live     : int64 [P * G], 0 or non-zero (the recording step's `unfinished` as it is), or NULL.
 *              A workgroup whose queries are all dead loads those words, writes zeros to their out
 *              rows and returns, before any barrier and before it forms an address into q, k, v
 *              or key_mask.  Otherwise a dead query gets zeros and its q row is not read.  A live
 *              query is bit-identical to the call without live.
 * Per query the floating-point operations and their order are those of trlx_t5_decode_attn: out is
 * bit-identical to trlx_t5_decode_attn on the keys, values and mask repeated G times, whatever the
 * strides and the tile.  G == 1 is that call.  The launch takes the same arguments at every token:
 * it captures as it is.
 * Refused with TRLX_ERR_ARG before any launch: a NULL a / q / k / v / out, a dtype other than
 * TRLX_F32 / TRLX_BF16, a d_kv other than 64 / 128, P, G, n_heads or S < 1, ldq below n_heads * d_kv
 * or not a whole number of 16-byte vectors, a stride that is negative or not a whole number of
 * 16-byte vectors, a head or key stride below d_kv, q / k / v / out not 16-byte aligned, key_mask /
 * live not 8-byte aligned, a P, G, n_heads or S whose grid would overflow. */
typedef struct TrlxT5DecodeAttnGroupArgs {
    const void* q;
    int64_t ldq;
    const void* k;
    int64_t k_stride_p, k_stride_h, k_stride_s;
    const void* v;
    int64_t v_stride_p, v_stride_h, v_stride_s;
    const int64_t* key_mask;          /* [P, S] int64, 0 = masked, or NULL */
    const int64_t* live;              /* [P * G] int64, 0 = skip, or NULL */
    void* out;                        /* [P * G, n_heads * d_kv], contiguous */
    int64_t P;
    int64_t G;
    int64_t n_heads;
    int64_t d_kv;                     /* 64 or 128 */
    int64_t S;
    int dtype;                        /* TRLX_F32 / TRLX_BF16: q, k, v, out */
} TrlxT5DecodeAttnGroupArgs;
int trlx_t5_decode_attn_group(const TrlxT5DecodeAttnGroupArgs* a, void* stream);

/* The largest query tile trlx_t5_decode_attn_group takes: 0 (the default: the measured choice, 4),
 * 1, 2, 4 or 8; anything else is refused with TRLX_ERR_ARG.  Process-wide.  A G below the tile
 * takes the smallest built tile that holds G.  The result does not depend on it; the benchmark
 * tool sets it to time each built tile. */
int trlx_t5_decode_attn_group_tile(int64_t tile);

/* ---------------------------------------------------------------- encoder keys split across workgroups
 * trlx_t5_decode_attn_group with the S keys of a (row, head) cut into X ranges, each walked by a
 * workgroup of its own: for the shapes where P * n_heads * tiles workgroups leave the chip
 * under-filled (few rows, few live rows) or S is long.  Opt-in: no other entry calls it.  The
 * arguments are trlx_t5_decode_attn_group's (G == 1 is the plain cross-attention) plus
 *   splits    : 0 = the X trlx_t5_decode_attn_split_plan returns for the shape, or 1 ... 8.
 *   workspace : device memory, 16-byte aligned, at least trlx_t5_decode_attn_split_workspace_bytes(
 *               P * G, n_heads, d_kv, X) bytes for the X taken; fp32 states [P * G, n_heads, ranges,
 *               d_kv + 2].  Scratch: nothing is kept in it between calls and it needs no
 *               initialisation; two calls in flight on different streams need a workspace each.
 * TWO launches in stream order, no atomics, no counters, no spinning:
 *   k_t5_decode_attn_split_part, grid (P * n_heads, tiles, ranges): the grouped kernel restricted to
 *     the keys [x * C, min(S, (x + 1) * C)), C = ceil(S / X) rounded up to a multiple of the
 *     kernel's NG groups (so key j is walked by group j % NG as in the unsplit kernel); only the
 *     ranges = ceil(S / C) non-empty ranges are launched.  Per live query it writes the
 *     unnormalised fp32 state (M, L, o[d_kv]); M = -inf, L = 0 when the range held no live key.
 *     A tile whose queries are all dead writes no state and forms no address into q, k, v or
 *     key_mask; a masked key's K and V rows are not read.
 *   k_t5_decode_attn_split_merge: M = max M_x; for every x with M_x != -inf, in split order,
 *     w = expf(M_x - M), L = fmaf(L_x, w, L), o = fmaf(o_x, w, o); out = o / L, or zeros when no key
 *     was live; one rounding.  A row with live[b] == 0 gets zeros and its states are not read.
 * The result is bit-reproducible and depends on X and on nothing else: not on P, the strides or
 * the query tile (trlx_t5_decode_attn_group_tile applies here as it does there).  X == 1 forwards to
 * trlx_t5_decode_attn_group: its bits.  For X > 1 the bits differ from the unsplit call's (the
 * groups are weighed against their range's maximum first), within the rounding of fp32 sums;
 * with a key_mask that leaves live keys in one range only they are the unsplit call's.  The
 * launches take the same arguments at every token: the call captures as it is.
 * Refused with TRLX_ERR_ARG before any launch: everything trlx_t5_decode_attn_group refuses, a
 * P * G * n_heads past 2^31 - 1, splits outside 0 ... 8, a workspace that is NULL, not 16-byte
 * aligned or smaller than the X taken needs (X == 1 included). */
int trlx_t5_decode_attn_split(const TrlxT5DecodeAttnGroupArgs* a, int64_t splits, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* Bytes of workspace for `rows` = P * G rows at `splits` ranges: rows * n_heads * splits *
 * (d_kv + 2) * 4.  0 for rows or n_heads < 1, a d_kv other than 64 / 128, splits outside 1 ... 8. */
int64_t trlx_t5_decode_attn_split_workspace_bytes(int64_t rows, int64_t n_heads, int64_t d_kv, int64_t splits);

/* The key ranges of trlx_t5_decode_attn_split for (dtype, d_kv, S) at `splits` (1 ... 8) ranges.  A host
 * function, no device needed.  TRLX_ERR_ARG (and a zeroed *g) for a NULL g, a dtype / d_kv the
 * kernels do not take, S < 1, splits outside 1 ... 8. */
typedef struct TrlxT5DecodeAttnSplitGeometry {
    int64_t NG;          /* groups of a workgroup: 32 / 16 / 16 / 8 for bf16-64 / bf16-128 / fp32-64 / fp32-128 */
    int64_t C;           /* keys a range: ceil(S / splits) rounded up to a multiple of NG */
    int64_t ranges;      /* non-empty ranges = ceil(S / C) <= splits: the grid's z and the states a (row, head) */
    int64_t tile;        /* the largest query tile in force (trlx_t5_decode_attn_group_tile) */
    int64_t max_splits;  /* 8 */
} TrlxT5DecodeAttnSplitGeometry;
int trlx_t5_decode_attn_split_geometry(int dtype, int64_t d_kv, int64_t S, int64_t splits,
                                       TrlxT5DecodeAttnSplitGeometry* g);

/* The X trlx_t5_decode_attn_split takes for splits == 0: a pure function of these arguments (it
 * looks neither at live nor at the device, so a shape always gives the same bits), in 1 ... 8, set
 * from measurements (profiles/t5_cross_split_bench.json).  1 for arguments the entry
 * would refuse. */
int trlx_t5_decode_attn_split_plan(int dtype, int64_t P, int64_t G, int64_t n_heads, int64_t d_kv, int64_t S);

/* The decoder's input row of decode step t, ONE launch — replaces, per generated token, the
 * gather of the token drawn at step t - 1, the `shared` embedding lookup (T5 applies no scale)
 * and layer 0's first T5LayerNorm.  clock == NULL: t is a->t; otherwise t and the capacity are
 * read from the decode clock (a->t is not read), once at the top of each workgroup.  Per row b:
 *   tok     = t == 0 ? start_token_id : tokens[b * ld_tokens + t - 1]
 *   h[b, :] = weight[tok, :], bit for bit; a tok outside [0, V) gives a zero row (tested before
 *             any address is formed from tok)
 *   y[b, :] = norm_w * h[b, :] * rsqrt(mean(h[b, :]^2) + eps), only with norm_w: bit-equal to
 *             trlx_t5_rmsnorm_fwd on h (the same row tile, sum order and kernel form by D); the
 *             row stays in registers between the gather and the two stores
 *   weight  : [V, D] of `dtype`, rows ld_w >= D elements apart (HF's shared.weight, or a slice of
 *             it, read in place)
 *   tokens  : int64 [B, T], rows ld_tokens >= T apart (the rollout record's tokens; a finished
 *             row holds pad there, which is what HF feeds)
 *   h, y    : [B, D] of `dtype`, rows ld_h / ld_y >= D apart; y NULL iff norm_w NULL
 * With a clock the step is live iff 0 <= t < clock T and t - 1 < a->T.  A dead step writes zeros
 * to h and y and reads neither tokens nor weight.  Stream-ordered, no sync, nothing allocated.
 * Refused before any launch, the outputs untouched — TRLX_ERR_ARG: a NULL a / weight / tokens /
 * h, y without norm_w or norm_w without y, a weight / h / y / norm_w not aligned to its element
 * or tokens / clock not aligned to 8 bytes, a NaN eps, a host t outside [0, T], h or y
 * overlapping any other operand; TRLX_ERR_SHAPE: D outside [1, 8192], B, V or T < 1;
 * TRLX_ERR_STRIDE: ld_w, ld_h or ld_y below D, ld_tokens below T; TRLX_ERR_DTYPE: a dtype other
 * than TRLX_F32 / TRLX_BF16. */
typedef struct TrlxT5DecodeEmbedArgs {
    const void* weight;               /* [V, D] */
    int64_t ld_w;
    const int64_t* tokens;            /* [B, T] */
    int64_t ld_tokens;
    const void* norm_w;               /* [D], or NULL: no y */
    void* h;                          /* [B, D] */
    int64_t ld_h;
    void* y;                          /* [B, D], or NULL */
    int64_t ld_y;
    int64_t B;
    int64_t D;                        /* 1..8192 */
    int64_t V;
    int64_t T;                        /* columns of tokens */
    int64_t t;                        /* host t in [0, T]; not read with a clock */
    int64_t start_token_id;           /* the token of t == 0 */
    float eps;
    int dtype;                        /* TRLX_F32 / TRLX_BF16: weight, norm_w, h, y */
} TrlxT5DecodeEmbedArgs;
int trlx_t5_decode_embed(const TrlxT5DecodeEmbedArgs* a, const int64_t* clock, void* stream);

/* ---------------------------------------------------------------- T5 full-sequence attention
 * Many queries against many keys under T5's rules, forward only — replaces the body of HF's
 * T5Attention between the q / k / v projections and the `o` projection (a [B, nH, Tq, S] matmul,
 * compute_bias, the additive mask, an fp32 softmax cast back, a second matmul) with ONE launch
 * that never holds a [Tq, S] tensor: a flash-attention forward on gfx950 MFMA, one workgroup per
 * (batch row, head, block of query rows).  bf16 only, d_kv 64 or 128.
 *   score[i, j] = q_i · k_j + bias_by_offset[h, (j - i) + (Tq - 1)]        (no 1/sqrt(d) scaling)
 *   out[b, i, h, :] = sum_j softmax_j(score[i, :]) * v_j   over the keys j that are not excluded
 *   q        : [B, Tq, n_heads, d_kv] as a base pointer + element strides for batch, position and
 *              head; the element stride is 1.  k, v: [B, S, n_heads, d_kv] likewise.  So a
 *              [B, T, nH * d] projection output (strides T*nH*d, nH*d, d), a slice of a fused
 *              [B, T, 3 * nH * d] projection and the cache layout [B, nH, S, d] (strides nH*S*d, d,
 *              S*d) are all read in place.  The stride of a dimension of size 1 is not read.
 *   out      : [B, Tq, n_heads, d_kv] with strides of its own; [B, Tq, nH * d] is what `o` takes.
 *   bias_by_offset : fp32 [n_heads, Tq + S - 1], contiguous, indexed by key position minus query
 *              position plus Tq - 1, or NULL (no bias).  Looked up inside the kernel.
 *   key_mask : int64 [B, S], contiguous, or NULL.  A key with key_mask[b, j] == 0 is excluded; its
 *              K and V rows are not read (they may hold anything, NaN included); a tile of keys
 *              with no live key is skipped.
 *   causal   : non-zero excludes the keys j > i and needs Tq == S; tiles of keys wholly above a
 *              block's last query are not read.
 * Both products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the scores, the bias add
 * and the online max / sum are fp32 and never rounded; P is rounded to bf16 un-normalised as the
 * P·V operand; O is rescaled in fp32 and rounded once at the end.  A query whose keys are all
 * excluded gives zeros (HF's additive finfo.min gives the plain average of the values there).
 * Tq and S may be any value >= 1: nothing outside [0, Tq) x [0, S) is read or written.  The
 * summation order depends on (d_kv, Tq, S, the flags, the mask row) only: the result is
 * bit-reproducible and does not depend on B or on the strides.
 * Refused with TRLX_ERR_ARG before any launch, `out` untouched: a dtype other than TRLX_BF16, a
 * d_kv other than 64 / 128, a NULL q / k / v / out, a base that is not 16-byte aligned, a stride
 * that is negative or no multiple of 8 elements, a position or head stride below d_kv, out rows
 * that overlap, causal with Tq != S, B, n_heads, Tq or S outside [1, 2^30], more than 2^31 - 1
 * workgroups, an operand whose last element lies beyond 2^61 elements from its base.
 * trlx_t5_attention_tiles reports the kernel's tile sizes (query rows per workgroup, keys per
 * LDS tile); either pointer may be NULL. */
typedef struct TrlxT5AttentionArgs {
    const void* q;
    int64_t q_stride_b, q_stride_t, q_stride_h;
    const void* k;
    int64_t k_stride_b, k_stride_t, k_stride_h;
    const void* v;
    int64_t v_stride_b, v_stride_t, v_stride_h;
    void* out;
    int64_t o_stride_b, o_stride_t, o_stride_h;
    const float* bias_by_offset;      /* [n_heads, Tq + S - 1] fp32, or NULL */
    const int64_t* key_mask;          /* [B, S] int64, 0 = excluded, or NULL */
    int64_t B;
    int64_t n_heads;
    int64_t d_kv;                     /* 64 or 128 */
    int64_t Tq;
    int64_t S;
    int dtype;                        /* TRLX_BF16 */
    int causal;
} TrlxT5AttentionArgs;
int trlx_t5_attention(const TrlxT5AttentionArgs* a, void* stream);
int trlx_t5_attention_tiles(int* q_tile, int* kv_tile);

/* The same launch, keeping the row statistics the backward needs.  `out` is bit-identical to
 * trlx_t5_attention's on the same arguments (the same kernel, one more store per query), and the
 * refusals are the same, plus a NULL or misaligned `lse`.
 *   lse : fp32 [B, n_heads, Tq], contiguous.  lse[b, h, i] = m_i + log(l_i) (natural log), m_i the
 *         largest live score of query i and l_i = sum_j exp(score[i, j] - m_i) over its live keys,
 *         so that exp(score[i, j] - lse) is the softmax weight.  A query with no live key gets +inf:
 *         exp(s - lse) is then 0 for every s and the backward gives it zero gradients. */
int trlx_t5_attention_fwd_lse(const TrlxT5AttentionArgs* a, float* lse, void* stream);

/* ---------------------------------------------------------------- T5 full-sequence attention, backward
 * The gradients of trlx_t5_attention (no dropout: the reference trains with dropout off) from
 * q, k, v, out, lse and dout, holding nothing of size Tq x S.  bf16 only, d_kv 64 or 128, both
 * products and their transposes on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  With
 * s = q_i · k_j + bias (unscaled) over the keys that are not excluded:
 *   P = exp(s - lse)      delta_i = sum_d dout_i · out_i      dP = dout · v^T      dS = P (dP - delta)
 *   dv = P^T · dout       dk = dS^T · q                       dq = dS · k
 *   dbias[h, (j - i) + Tq - 1] = sum over b and the live (i, j) of dS[b, h, i, j]
 * P and dS are fp32 and rounded to bf16 only as MFMA operands; dq, dk, dv are rounded once.
 * Three launches: delta (a row kernel), dk / dv (one workgroup per batch row, head and block of
 * keys, walking the queries), dq (one workgroup per batch row, head and block of queries, walking
 * the keys; it also sums dbias).  The scores are recomputed in both walks: dq, dk and dv use no
 * global atomics, their summation order depends on (d_kv, Tq, S, the flags, the mask row) only, so
 * they are bit-reproducible run to run and do not depend on B or on the strides.
 *   q, k, v, out, dout : as in TrlxT5AttentionArgs, base pointer + element strides for batch,
 *              position and head, read in place (dout: [B, Tq, n_heads, d_kv]).
 *   dq, dk, dv : written with three strides of their own each, shaped like q, k, v; e.g. the three
 *              slices of one fused [B, T, 3 * nH * d] gradient buffer.
 *   lse      : trlx_t5_attention_fwd_lse's, fp32 [B, n_heads, Tq], contiguous.
 *   bias_by_offset, key_mask, causal : the forward's.  The K and V rows of excluded keys are not
 *              read; their dk and dv rows are written as exact zeros.  Tiles with no live key and
 *              tiles above the causal diagonal are skipped.  dq of a query with no live key is
 *              exact zeros.  Nothing outside [0, Tq) x [0, S) is read or written, Tq, S >= 1.
 *   dbias    : fp32 [n_heads, Tq + S - 1], contiguous, or NULL (not computed, nothing paid: the
 *              bias belongs to a frozen layer).  The call zeroes it, then accumulates with LDS and
 *              global fp32 atomics: dbias is NOT bit-reproducible (dq, dk, dv are the same bits
 *              with and without it).  It may be given without bias_by_offset (the bias is 0 then).
 *   workspace : trlx_t5_attention_bwd_workspace_bytes(B, n_heads, Tq) bytes (delta, fp32
 *              [B, n_heads, Tq]; it does not grow with S), 4-byte aligned; -1 for sizes out of range.
 * Refused with TRLX_ERR_ARG before any launch, every output untouched: the forward's list (for
 * out as a read operand), a NULL dout / lse / dq / dk / dv, a misaligned base, dq / dk / dv rows
 * that overlap within one of them, a dq / dk / dv that shares an element with another of them or
 * with q / k / v / out / dout (operands whose address ranges interleave, such as the slices of one
 * fused buffer, are told apart exactly when their sizes and strides are equal and refused
 * otherwise), a missing or short workspace.  dbias, lse and the workspace are the caller's to keep
 * apart from the rest.
 * trlx_t5_attention_bwd_tiles reports the tiles: the dq kernel's query rows per workgroup and keys
 * per LDS tile, the dk / dv kernel's keys per workgroup and query rows per LDS tile; any pointer
 * may be NULL.  Not built: dropout, fp32 / fp16, other d_kv, causal with a cached prefix, a double
 * backward, a single-kernel backward with atomically accumulated dq. */
typedef struct TrlxT5AttentionBwdArgs {
    const void* q;
    int64_t q_stride_b, q_stride_t, q_stride_h;
    const void* k;
    int64_t k_stride_b, k_stride_t, k_stride_h;
    const void* v;
    int64_t v_stride_b, v_stride_t, v_stride_h;
    const void* out;
    int64_t o_stride_b, o_stride_t, o_stride_h;
    const void* dout;
    int64_t do_stride_b, do_stride_t, do_stride_h;
    void* dq;
    int64_t dq_stride_b, dq_stride_t, dq_stride_h;
    void* dk;
    int64_t dk_stride_b, dk_stride_t, dk_stride_h;
    void* dv;
    int64_t dv_stride_b, dv_stride_t, dv_stride_h;
    const float* lse;                 /* [B, n_heads, Tq] fp32 */
    const float* bias_by_offset;      /* [n_heads, Tq + S - 1] fp32, or NULL */
    const int64_t* key_mask;          /* [B, S] int64, 0 = excluded, or NULL */
    float* dbias;                     /* [n_heads, Tq + S - 1] fp32, or NULL */
    void* workspace;
    int64_t workspace_bytes;
    int64_t B;
    int64_t n_heads;
    int64_t d_kv;                     /* 64 or 128 */
    int64_t Tq;
    int64_t S;
    int dtype;                        /* TRLX_BF16 */
    int causal;
} TrlxT5AttentionBwdArgs;
int trlx_t5_attention_bwd(const TrlxT5AttentionBwdArgs* a, void* stream);
int64_t trlx_t5_attention_bwd_workspace_bytes(int64_t B, int64_t n_heads, int64_t Tq);
int trlx_t5_attention_bwd_tiles(int* dq_q_tile, int* dq_kv_tile, int* dkv_k_tile, int* dkv_q_tile);

/* ---------------------------------------------------------------- T5 feed-forward activation
 * What sits between the projections of HF's T5LayerFF, forward and backward, one launch each:
 *   forward   out[n, f] = act(u[n, f]) * v[n, f]        (T5DenseGatedActDense: u = wi_0(x), v = wi_1(x))
 *             out[n, f] = act(u[n, f])                  with v NULL (T5DenseActDense)
 *   backward  du = dy * v * act'(u)     dv = dy * act(u)     (du = dy * act'(u) with v NULL)
 * act: TRLX_T5_ACT_RELU, TRLX_T5_ACT_GELU_NEW (0.5 u (1 + tanh(sqrt(2/pi) (u + 0.044715 u^3))), HF's
 * `gelu_new`, what `gated-gelu` maps to; not the erf GELU) or TRLX_T5_ACT_SILU.  TRLX_F32 or TRLX_BF16,
 * one dtype for every operand; all arithmetic in fp32, every output rounded once.  gelu_new and silu
 * are evaluated as u * sigmoid(x) (x = u, or 2 sqrt(2/pi) (u + 0.044715 u^3)) from e = exp(-|x|):
 * nothing cancels, every finite input gives a finite output and derivative (1 towards +inf, 0
 * towards -inf), a NaN element gives NaN in that element only.  relu'(0) = 0.  The backward
 * recomputes act(u); it reads dy, u and v and nothing else.
 *   u, v, out, dy, du, dv : rows of F elements with element stride 1 and a row stride (in elements)
 *             of their own each, ld_* >= F (checked for every N): the halves of a packed [N, 2F]
 *             projection output are read in place, du and dv can be the halves of one [N, 2F]
 *             gradient.  The forward takes u, v, out; the backward u, v, dy, du, dv.
 *   du, dv  : either may be NULL (not computed, nothing paid), not both; dv needs v; with du NULL
 *             v is not read.
 * 16-byte accesses when every base pointer of the call is 16-byte aligned and F and every row
 * stride are multiples of the vector width (8 bf16, 4 fp32); element accesses otherwise.  The two
 * forms give the same bits.  No workspace, no atomics: bit-reproducible.  N == 0 is a success with
 * no launch.
 * Refused before any launch, every output untouched: NULL args, a NULL u / out (forward) or
 * u / dy (backward), du and dv both NULL, dv without v (TRLX_ERR_ARG); F <= 0, N < 0, sizes past
 * the grid (TRLX_ERR_SHAPE); a row stride below F (TRLX_ERR_STRIDE); a dtype other than the two
 * (TRLX_ERR_DTYPE); an unknown act, a pointer not aligned to its element, a written operand that
 * shares an element with any other operand (TRLX_ERR_ARG; operands whose address ranges interleave,
 * such as the halves of one packed buffer, are told apart exactly when their row strides are equal
 * and refused otherwise, the rule of trlx_t5_attention_bwd).
 * trlx_t5_ff_act_geometry reports the vector widths and the block of columns and rows one
 * workgroup takes; any pointer may be NULL.  Not built: the erf GELU, fp16, dropout, the
 * projections themselves. */
typedef enum {
    TRLX_T5_ACT_RELU = 0,
    TRLX_T5_ACT_GELU_NEW = 1,
    TRLX_T5_ACT_SILU = 2,
} trlx_t5_act;
typedef struct TrlxT5FfActArgs {
    const void* u;
    int64_t ld_u;
    const void* v;                    /* NULL = not gated */
    int64_t ld_v;
    void* out;                        /* forward only */
    int64_t ld_out;
    const void* dy;                   /* backward only */
    int64_t ld_dy;
    void* du;                         /* backward only, or NULL */
    int64_t ld_du;
    void* dv;                         /* backward only, or NULL */
    int64_t ld_dv;
    int64_t N;
    int64_t F;
    int dtype;                        /* TRLX_F32 / TRLX_BF16 */
    int act;                          /* trlx_t5_act */
} TrlxT5FfActArgs;
int trlx_t5_ff_act_fwd(const TrlxT5FfActArgs* a, void* stream);
int trlx_t5_ff_act_bwd(const TrlxT5FfActArgs* a, void* stream);
int trlx_t5_ff_act_geometry(int* vec_bf16, int* vec_f32, int* cols_per_block, int* rows_per_block);

/* ---------------------------------------------------------------- T5 RMSNorm with the residual add
 * HF's T5LayerNorm (no mean subtraction, no bias, eps inside the root) and the residual add of the
 * sub-layer before it (T5LayerFF / T5LayerSelfAttention: hidden + sublayer(norm(hidden))):
 *   forward   h[n, j] = residual[n, j] + x[n, j]         add form only (residual and h given); rounded once
 *             rstd[n] = 1 / sqrt(mean_j h[n, j]^2 + eps)  fp32, from h as rounded (without residual, x is h)
 *             y[n, j] = w[j] * (h[n, j] * rstd[n])        fp32 arithmetic, rounded once
 *   backward  g = w dy,  hh = h rstd,  c[n] = mean_j g hh
 *             dh[n, j] = rstd[n] (g[n, j] - hh[n, j] c[n]) + dh_in[n, j]      rounded once
 *             dw[j]    = sum_n dy[n, j] hh[n, j]                               fp32 sum, rounded once
 * TRLX_F32 or TRLX_BF16, one dtype for every operand, w and dw included; rstd and ws are fp32.
 *   x, residual, h, y, dy, dh_in, dh : N rows of D elements, element stride 1 and a row stride (in
 *             elements) of their own each, ld_* >= D (checked for every N): h[:, -1, :], a [B, 1, D]
 *             decode slice and padded buffers are read in place.  1 <= D <= 8192 (a row stays in
 *             registers from the sum of squares to the stores: it is read once).
 *   forward   reads x (and residual), writes y (and h), and rstd [N] when it is not NULL: one launch.
 *             h may be the very rows of residual or of x (same pointer, same stride): the add in
 *             place.  Without residual, y may be the very rows of x.  h never overlaps y, and no
 *             other overlap of a written operand with another operand is taken.
 *   backward  reads dy, h, and w (for dh), dh_in when not NULL, rstd when not NULL (else it is
 *             recomputed from h).  dh and dw: either may be NULL (not computed, not written), not
 *             both.  dh: one launch.  dw: the row launch leaves one fp32 partial row per workgroup in
 *             ws [G, D] (every element the second launch reads was written: ws needs no clearing),
 *             a second launch adds the G rows of a column in a fixed order: no atomics,
 *             bit-reproducible.  ws_bytes >= trlx_t5_rmsnorm_geometry's ws_bytes for (N, D); with
 *             dw NULL ws is not looked at.  dh may be the very rows of dh_in or of dy.
 * 16-byte accesses when every pointer of the call is 16-byte aligned and D and every row stride are
 * multiples of the vector width (8 bf16, 4 fp32); element accesses otherwise.  The two forms give
 * the same bits.  N == 0 is a success (dw, if asked for, is cleared).
 * Rows: an all-zero row gives y = 0 and rstd = eps^-1/2; a row whose sum of squares overflows fp32
 * gives rstd = 0 and y = 0 as HF's fp32 expression does; a NaN stays in its row (y, dh) and reaches dw.
 * Refused before any launch, every output untouched: NULL args or a NULL required pointer, residual
 * without h or h without residual, dh and dw both NULL, dh_in without dh, a workspace that is NULL,
 * misaligned or too small, a pointer not aligned to its element, h overlapping y or any other
 * overlap not named above (TRLX_ERR_ARG); D outside [1, 8192], N < 0 (TRLX_ERR_SHAPE); a row stride
 * below D (TRLX_ERR_STRIDE); a dtype other than the two (TRLX_ERR_DTYPE).
 * trlx_t5_rmsnorm_geometry fills the launch geometry; the per-shape fields are 0 when D is outside
 * [1, max_d].  Not built: fp16, dropout, a double backward; the norm fused into a projection exists for
 * decode steps only (trlx_t5_decode_linear). */
typedef struct TrlxT5RmsNormArgs {
    const void* x;                    /* forward: the sub-layer output (add form) or the rows to normalise */
    int64_t ld_x;
    const void* residual;             /* forward, add form only, or NULL */
    int64_t ld_residual;
    void* h;                          /* forward: written in the add form, NULL otherwise; backward: read */
    int64_t ld_h;
    void* y;                          /* forward only */
    int64_t ld_y;
    const void* dy;                   /* backward only */
    int64_t ld_dy;
    const void* dh_in;                /* backward only, or NULL */
    int64_t ld_dh_in;
    void* dh;                         /* backward only, or NULL */
    int64_t ld_dh;
    const void* w;                    /* [D] */
    void* dw;                         /* backward only, [D], or NULL */
    void* rstd;                       /* fp32 [N]: written by the forward, read by the backward, or NULL */
    void* ws;                         /* backward with dw: fp32 [G, D] */
    int64_t ws_bytes;
    int64_t N;
    int64_t D;
    float eps;
    int dtype;                        /* TRLX_F32 / TRLX_BF16 */
} TrlxT5RmsNormArgs;
typedef struct TrlxT5RmsNormGeometry {
    int vec_bf16, vec_f32;            /* elements per 16-byte access */
    int threads;                      /* per workgroup */
    int max_partials;                 /* the cap of G */
    int max_d;                        /* the largest D taken */
    int reg_max_d;                    /* the largest D whose row stays in registers (= max_d) */
    int wave_row_max_d;               /* up to here one wave takes a row, threads / 64 rows per workgroup pass; above, one row */
    int n_breaks;
    int d_breaks[8];                  /* ascending: the largest D of each kernel form (elements per thread, wave or workgroup per row) */
    int rows_per_block;               /* for this D: rows per workgroup pass */
    int reserved;
    int64_t row_blocks;               /* ceil(N / rows_per_block) */
    int64_t partials;                 /* G = min(row_blocks, max_partials): workgroups of either row launch */
    int64_t ws_bytes;                 /* G * D * 4 */
} TrlxT5RmsNormGeometry;
int trlx_t5_rmsnorm_fwd(const TrlxT5RmsNormArgs* a, void* stream);
int trlx_t5_rmsnorm_bwd(const TrlxT5RmsNormArgs* a, void* stream);
int trlx_t5_rmsnorm_geometry(int64_t N, int64_t D, TrlxT5RmsNormGeometry* g);

/* ---------------------------------------------------------------- T5 decode-step projection
 * One projection of a decode step with its neighbours in the same launch (opt-in; the projections
 * of every other path stay hipBLASLt):
 *   out[m, n] = epilogue( sum_k xh[m, k] * weight[n, k] )      bf16 MFMA, fp32 accumulation
 *   prologue  norm_weight NULL: xh = x.  Else T5's RMSNorm in front of the projection:
 *             xh[m, k] = bf16(norm_weight[k] * (x[m, k] * rstd[m])), rstd[m] = 1 / sqrt(mean_k x[m, k]^2 + eps),
 *             the sum order, the product and the one rounding of trlx_t5_rmsnorm_fwd for D = K, so xh
 *             has the bits of that forward on x; the normed rows are never written.  K <= 8192.
 *   epilogue  at most one of
 *             residual [M, N]  : out = bf16(acc + residual), one rounding.  out may be the very rows of
 *                                residual (same pointer, same stride): the stream updated in place.
 *             act, gated = 0   : out = bf16(act(acc)), weight [N, K]               (T5DenseActDense's wi)
 *             act, gated = 1   : weight is [2N, K], wi_0's rows then wi_1's; out[m, j] =
 *                                bf16(act(u) * v) with u, v the fp32 accumulators of weight rows j and
 *                                N + j                                       (T5DenseGatedActDense)
 *             act is a trlx_t5_act evaluated as trlx_t5_ff_act_fwd evaluates it, or TRLX_T5_ACT_NONE.
 *   x       : [M, K], element stride 1, row stride ld_x >= K (h[:, -1, :] is read in place)
 *   weight  : nn.Linear.weight layout, rows of K elements ld_w >= K apart
 *   out     : [M, N], row stride ld_out >= N.  N counts output columns in every form.
 * TRLX_BF16 only.  M >= 1; K a multiple of 32, 32 to 16384; N a multiple of 16.  Every pointer is
 * 16-byte aligned and every row stride a multiple of 8 elements.
 * A workgroup owns 16 output columns and every row; K is split across the four waves of the
 * workgroup only and their partial sums are added in wave order: no atomics, no workspace, two calls
 * give the same bits.  No allocation and no host read: the call is the same launch at every token
 * and can be captured.
 * Refused before any launch, out untouched: NULL args / x / weight / out, a pointer off the 16-byte
 * grid, an unknown act, gated without an act, a residual together with an act, a NaN eps, out sharing
 * a byte range with x, weight or norm_weight, or with residual other than as the very same rows
 * (TRLX_ERR_ARG); M, K or N off the grid above, K > 8192 with a norm weight (TRLX_ERR_SHAPE); a row
 * stride below the row or off the 16-byte grid (TRLX_ERR_STRIDE); a dtype other than TRLX_BF16
 * (TRLX_ERR_DTYPE).
 * trlx_t5_decode_linear_geometry reports the blocking.  Not built: fp32 / fp16, a backward, a bias,
 * K split across workgroups. */
#define TRLX_T5_ACT_NONE (-1)
typedef struct trlx_t5_decode_linear_args {
    const void* x;
    int64_t ld_x;
    const void* weight;
    int64_t ld_w;
    const void* norm_weight;          /* [K] or NULL */
    const void* residual;             /* [M, N] or NULL */
    int64_t ld_residual;
    void* out;
    int64_t ld_out;
    int64_t M;
    int64_t K;
    int64_t N;                        /* output columns */
    float eps;
    int dtype;                        /* TRLX_BF16 */
    int act;                          /* trlx_t5_act or TRLX_T5_ACT_NONE */
    int gated;                        /* weight is [2N, K] */
} trlx_t5_decode_linear_args;
typedef struct TrlxT5DecodeLinearGeometry {
    int threads;                      /* per workgroup */
    int cols_per_block;               /* output columns a workgroup owns */
    int rows_per_tile;
    int k_per_chunk;                  /* K of one MFMA */
    int chunks_per_wave_turn;         /* chunk c belongs to wave (c / this) % (threads / 64) */
    int max_row_tiles;                /* accumulator tiles of a wave: row tiles per pass x weight slabs */
    int max_k;
    int norm_max_k;                   /* the largest K taken with a norm weight */
    int norm_wave_row_max_k;          /* up to here the norm's sum takes one wave per row */
    int reserved;
} TrlxT5DecodeLinearGeometry;
int trlx_t5_decode_linear(const trlx_t5_decode_linear_args* a, void* stream);
int trlx_t5_decode_linear_geometry(TrlxT5DecodeLinearGeometry* g);

/* The same projection with the rows spread over workgroups and a skip of finished rows (opt-in;
 * csrc/t5_decode_linear_rows.hip).  The expression, the eight epilogue forms, the norm prologue and
 * the per-tile arithmetic are trlx_t5_decode_linear's; the grid is (N / 16, ceil(M / rows_per_block))
 * and a workgroup owns 16 output columns and ONE block of rows_per_block rows.  A row's output does
 * not depend on the tile or workgroup it lands in: every live row has the bits
 * trlx_t5_decode_linear gives it.
 *   live : NULL (every row live), or device int64 [M], nonzero = live (the rollout recorder's
 *          `unfinished` as it is), read on the device: the launch is the same at every token.  The
 *          live rows are compacted in row order, rows_per_block of them per workgroup; a workgroup
 *          without live rows loads no weight.  A dead row behaves as a zero input row and nothing of
 *          x is read for it: out[m] = 0 in the plain, norm and activation forms; out[m] = residual[m]
 *          in the residual form; left untouched when out is the residual.  Every element of out is
 *          written exactly once per call (an in-place dead row: not at all).
 * No atomics, no workspace, no allocation; K is never split across workgroups; two calls give the
 * same bits.
 * Refused before any launch, out untouched: everything trlx_t5_decode_linear refuses, with its
 * statuses; live off the 8-byte grid or sharing a byte range with out (TRLX_ERR_ARG); M above
 * 65535 * rows_per_block (the grid's second dimension), or above max_m_live = 4096 with live
 * (TRLX_ERR_SHAPE).  max_m_live is a bound on a cost, not on the scan, which would run for any M:
 * every workgroup reads up to M live words from L2, 32 KB at 4096 rows, and only M 256 is measured.
 * trlx_t5_decode_linear_rows_geometry is a host call and needs no device. */
typedef struct trlx_t5_decode_linear_rows_args {
    const void* x;
    int64_t ld_x;
    const void* weight;
    int64_t ld_w;
    const void* norm_weight;          /* [K] or NULL */
    const void* residual;             /* [M, N] or NULL */
    int64_t ld_residual;
    void* out;
    int64_t ld_out;
    int64_t M;
    int64_t K;
    int64_t N;                        /* output columns */
    float eps;
    int dtype;                        /* TRLX_BF16 */
    int act;                          /* trlx_t5_act or TRLX_T5_ACT_NONE */
    int gated;                        /* weight is [2N, K] */
    const int64_t* live;              /* device int64 [M], nonzero = live, or NULL */
    int64_t reserved;                 /* 0 */
} trlx_t5_decode_linear_rows_args;
typedef struct TrlxT5DecodeLinearRowsGeometry {
    int threads;                      /* per workgroup */
    int cols_per_block;               /* output columns a workgroup owns */
    int rows_per_tile;
    int rows_per_block;               /* rows a workgroup owns: the grid's second dimension is ceil(M / this) */
    int max_m_live;                   /* the largest M taken with live */
    int reserved;
} TrlxT5DecodeLinearRowsGeometry;
int trlx_t5_decode_linear_rows(const trlx_t5_decode_linear_rows_args* a, void* stream);
int trlx_t5_decode_linear_rows_geometry(TrlxT5DecodeLinearRowsGeometry* g);

/* ---------------------------------------------------------------- §8f: device-resident rollout store
 * Row copy between padded columnar [rows, W] buffers — replaces the reference's
 * `.cpu()` of the experience tensors, per-sample PPORLElement lists and the pad_sequence
 * collate (ppo_orchestrator.py:169-187, ppo_pipeline.py:36-66).  For each of nfields
 * (<= 8) fields i, for j < rows and c < cols[i]:
 *   dst[i][drow(j) * dst_ld[i] + dst_col0[i] + c] = src[i][srow(j) * src_ld[i] + src_col0[i] + c]
 * srow(j) = src_idx ? src_idx[j] : src_row0 + j (drow likewise); element size esize[i] in
 * {2, 4, 8} bytes; strides / columns in elements.  The host arrays are read during the call
 * only; src_idx / dst_idx are device int64 vectors. */
int trlx_rows_copy(int nfields, const void* const* src, void* const* dst, const int64_t* src_ld,
                   const int64_t* dst_ld, const int64_t* src_col0, const int64_t* dst_col0,
                   const int64_t* cols, const int* esize, int64_t rows, const int64_t* src_idx,
                   int64_t src_row0, const int64_t* dst_idx, int64_t dst_row0, void* stream);

/* decoder_input_ids of the seq2seq policy forward from a collated response batch — replaces
 * shift_tokens_right (trlx/model/accelerate_ppo_model.py:18-25) as called by
 * AcceleratePPOModel.get_model_inputs (:63-76): out[b,0] = decoder_start_token_id,
 * out[b,t] = ids[b,t-1], then every -100 -> pad_token_id.  ids / out: device int64 [B, T] with
 * row strides ld / out_ld (unit column stride), out must not alias ids; T >= 1 (the reference
 * raises IndexError on an empty response), B = 0 is a no-op. */
int trlx_shift_tokens_right(const int64_t* ids, int64_t B, int64_t T, int64_t ld, int64_t pad_token_id,
                            int64_t decoder_start_token_id, int64_t* out, int64_t out_ld, void* stream);

/* ---------------------------------------------------------------- §8f: device-resident ILQL rollout store
 * The offline dataset of ILQLRolloutStorage (trlx/pipeline/offline_pipeline.py:57-85) as six
 * flat device buffers in three offset families, each with an int64 prefix-sum vector of
 * N + 1 entries (sample i of family X spans [off_X[i], off_X[i+1]), len_X(i) its length):
 *   off_L: input_ids, attention_mask     off_S: states_ixs, dones     off_A: actions_ixs, rewards
 * rewards is fp32, the other five fields are int64.
 *
 * trlx_ilql_collate builds one training batch in one launch — replaces the pad_sequence
 * collate_fn (offline_pipeline.py:88-108) and to_device(batch) (accelerate_ilql_model.py:58-68).
 * For each field f of family X, j < n and c < W_X:
 *   out_f[j * ld_f + c] = c < len_X(idx[j]) ? f[off_X[idx[j]] + c] : 0
 * idx: device int64 [n] sample numbers, any order, repeats allowed; an entry outside [0, N)
 * gives a row of pads and reads nothing.  Columns >= W_X are never written (a longer sample is
 * truncated, row strides ld_f >= W_X in elements), length 0 gives a row of pads, an output of
 * width 0 may be NULL, n = 0 is a no-op. */
int trlx_ilql_collate(const int64_t* input_ids, const int64_t* attention_mask, const float* rewards,
                      const int64_t* states_ixs, const int64_t* actions_ixs, const int64_t* dones,
                      const int64_t* off_L, const int64_t* off_S, const int64_t* off_A, int64_t N,
                      const int64_t* idx, int64_t n, int64_t WL, int64_t WS, int64_t WA,
                      int64_t* out_input_ids, int64_t ld_input_ids, int64_t* out_attention_mask,
                      int64_t ld_attention_mask, float* out_rewards, int64_t ld_rewards,
                      int64_t* out_states_ixs, int64_t ld_states_ixs, int64_t* out_actions_ixs,
                      int64_t ld_actions_ixs, int64_t* out_dones, int64_t ld_dones, void* stream);

/* The device half of OfflineOrchestrator.make_experience (offline_orchestrator.py:39-70): the
 * five derived flat fields of all N samples in one launch.  Sample i with prompt_len[i] = p:
 *   attention_mask = 1 (len_L)          states_ixs = p-1, p, ... (len_S)     actions_ixs = p-1, p, ... (len_A)
 *   dones = 1 ... 1 0 (len_S)           out_rewards = 0 ... 0 G_i (len_A)
 *   G_i = (rewards[i] - mean) / (std + 1e-30), unbiased std, evaluated in fp64 and rounded to fp32
 * mean / std come from stats[4] = {sum, sumsq, count, .} of the raw rewards
 * (trlx_moments_partial / trlx_moments_finalize), read on the device; count 1 gives NaN as
 * torch's std() does.  The caller makes the offsets consistent (len_S = len_L - p + 1,
 * len_A = len_L - p, 1 <= p < len_L); total_X = off_X[N] is the length of family X's buffers,
 * past which nothing is written whatever the offsets hold.  N = 0 is a no-op. */
int trlx_ilql_build_fields(const int64_t* off_L, const int64_t* off_S, const int64_t* off_A,
                           const int64_t* prompt_len, const float* rewards, const double* stats, int64_t N,
                           int64_t total_L, int64_t total_S, int64_t total_A, int64_t* attention_mask,
                           int64_t* states_ixs, int64_t* actions_ixs, int64_t* dones, float* out_rewards,
                           void* stream);

/* ---------------------------------------------------------------- §8f rank 4: device-resident controller state
 * The PPO loop's host scalars — RunningMoments of the scores (trlx/utils/modeling.py:72-104),
 * the orchestrator's ref_mean/ref_std + score scale/clip (ppo_orchestrator.py:48-49,96-112)
 * and the KL coefficient of Adaptive/FixedKLController (ppo_models.py:26-58) — as ONE fp64
 * record in device memory, read and advanced in-stream (no host synchronisation).
 * Slots (doubles): */
#define TRLX_CTL_SLOTS 16
#define TRLX_CTL_MEAN 0          /* RunningMoments.mean  */
#define TRLX_CTL_VAR 1           /* RunningMoments.var   */
#define TRLX_CTL_STD 2           /* RunningMoments.std   */
#define TRLX_CTL_COUNT 3         /* RunningMoments.count */
#define TRLX_CTL_REF_MEAN 4      /* orchestrator ref_mean */
#define TRLX_CTL_REF_STD 5       /* orchestrator ref_std  */
#define TRLX_CTL_REF_SET 6       /* 1 once ref_mean is known (config or first batch) */
#define TRLX_CTL_KL_COEF 7       /* kl_ctl.value (beta) */
#define TRLX_CTL_BATCH_MEAN 8    /* last RunningMoments.update return values */
#define TRLX_CTL_BATCH_STD 9
#define TRLX_CTL_KL_UPDATES 10   /* number of kl_ctl.update calls */
#define TRLX_CTL_LAST_KL 11      /* last approx_kl given to kl_ctl.update */

typedef enum {
    TRLX_SCALE_NONE = 0,     /* scale_reward False */
    TRLX_SCALE_RUNNING = 1,  /* "running": scores /= running.std */
    TRLX_SCALE_REF = 2,      /* "ref": scores /= ref_std */
} trlx_scale_mode;

/* Score-side control: RunningMoments.update(scores) (global moments when given: the
 * all-reduced {Σx, Σx², n} of trlx_score_moments over ranks, else the local batch), the
 * first-batch ref_mean/ref_std, then scores = clip(scores / scale, ±cliprange_reward). */
typedef struct {
    const double* state_in;          /* [TRLX_CTL_SLOTS] */
    double* state_out;               /* [TRLX_CTL_SLOTS], may equal state_in only in trlx_score_ctl_update */
    const double* global_moments;    /* [>=3] or NULL */
    int scale_mode;                  /* trlx_scale_mode */
    float cliprange_reward;          /* 0 = no clip */
} trlx_score_ctl;

/* KL-side control: kl_ctl.update(approx_kl, n_steps) on state (in place). */
typedef struct {
    double* state;                   /* [TRLX_CTL_SLOTS] */
    int adaptive;                    /* 1 AdaptiveKLController, 0 FixedKLController */
    double target, horizon;
    int64_t n_steps;                 /* config.train.batch_size (accelerate_ppo_model.py:131) */
} trlx_kl_ctl;

/* state = {mean 0, var 1, std 1, count 1e-24, ref_mean, ref_std, ref_set, init_kl_coef, ...}
 * (RunningMoments.__init__, modeling.py:78-81; orchestrator :48-49; kl_ctl init). */
int trlx_ctl_init(double* state, double init_kl_coef, double ref_mean, double ref_std, int ref_set,
                  void* stream);
/* {Σx, Σx², n, 0} of scores (fp64, one workgroup) — the record a caller all-reduces across
 * ranks before trlx_score_ctl_update / trlx_ppo_rollout_gae_ctl. */
int trlx_score_moments(const void* scores, int dtype, int64_t n, double* moments, void* stream);
/* trlx_score_moments with `done_event` (a hipEvent_t) recorded by the kernel's own dispatch
 * (hipExtLaunchKernel stop event) instead of a separate hipEventRecord marker between this
 * launch and the next: the ordering point the RCCL helper's side stream waits on before the
 * score-moments all-reduce. */
int trlx_score_moments_signal(const void* scores, int dtype, int64_t n, double* moments, void* stream,
                              void* done_event);
/* One workgroup: the score-side control above; scores_out (may alias scores) receives the
 * scaled, clipped scores.  ppo_orchestrator.py:96-112. */
int trlx_score_ctl_update(const void* scores, int dtype, int64_t n, const trlx_score_ctl* ctl,
                          void* scores_out, int out_dtype, void* stream);
/* kl_ctl.update with approx_kl read from device memory (fp32, e.g. the loss stats slot 8). */
int trlx_kl_ctl_update(const trlx_kl_ctl* kl, const float* approx_kl, void* stream);
/* The fused step's tails with the controller state folded in (no extra launch):
 *   trlx_ppo_rollout_gae_ctl  = trlx_ppo_rollout_gae with beta read from ctl->state_in and
 *                               the scores passed through the score-side control (every
 *                               block derives the same values; block 0 writes state_out,
 *                               which must not alias state_in);
 *   trlx_ppo_rollout_loss_ctl = trlx_ppo_rollout_loss + kl_ctl.update(approx_kl) by the
 *                               block that writes the stats. */
int trlx_ppo_rollout_gae_ctl(int64_t B, int64_t T, const float* lp, const float* ref_lp, const void* values,
                             int v_dtype, const float* scores, const int64_t* lengths, const int64_t* mask,
                             const trlx_score_ctl* ctl, double gamma, double lam, float* rewards, float* adv_raw,
                             void* ret, int ret_dtype, double* stats, void* workspace, void* stream);
int trlx_ppo_rollout_loss_ctl(int64_t B, int64_t T, const double* stats, float vf_coef, float* loss,
                              float* loss_stats, void* workspace, const trlx_kl_ctl* kl, void* stream);
/* trlx_lsm_gather_fwd (the next step's experience rows) with the PREVIOUS step's loss tail
 * (trlx_ppo_rollout_loss[_ctl] over tail_B x tail_T token records of `workspace`; kl may be
 * NULL) folded in as the launch's first workgroups: the tail's ~9 us latency-bound
 * reduction and its launch leave the critical path and no cross-stream event is needed.
 * Kernels that cannot host it (the streaming rows) run the tail as its own launch first.
 * Stream order is that of the two calls: the tail reads the token records of the loss rows
 * launched before, the GAE tail launched after reads the KL coefficient it updates.
 * lengths, order_ws: as in trlx_lsm_gather_fwd_ragged (NULL: every row / natural order). */
int trlx_lsm_gather_fwd_loss_tail(const void* x0, const void* x1, int dtype, int64_t B, int64_t T, int64_t V,
                                  int64_t sb, int64_t st, const int64_t* labels, int64_t lb, int64_t lt,
                                  const int64_t* lengths, void* order_ws, void* out_lp0, void* out_lp1, int out_dtype,
                                  int64_t tail_B, int64_t tail_T,
                                  const double* tail_stats, float vf_coef, float* loss, float* loss_stats,
                                  void* workspace, const trlx_kl_ctl* kl, void* stream);

/* ---------------------------------------------------------------- split-beta step (DP pipeline)
 * The KL-penalised reward r = score_t - beta*kl_t (ppo_orchestrator.py:163-167) enters GAE
 * (ppo_models.py:121-139) linearly, so A = A0 - beta*Ak with A0 the GAE of the score +
 * value terms and Ak the discounted KL sums.  Splitting them lets the GAE launch run before
 * the previous batch's KL-controller update (accelerate_ppo_model.py:123,130-131), which the
 * pipelined data-parallel schedule needs to keep its loss tail folded.
 *   trlx_ppo_rollout_gae_split  one wave per rollout: adv0 = A0, adv_kl = Ak, rew_kl = kl_t
 *       (0 past the length), rew_score = the score term (-0.0 before the last column, 0 past
 *       it) and the split record stats8 = {Σ A0, Σ A0², n, Σ Ak, Σ A0·Ak, Σ Ak², Σ mask, 0}
 *       (all-reduce the first 6, or 7 for a global loss normaliser).  ctl: score control as
 *       in trlx_ppo_rollout_gae_ctl (may be NULL); beta is not read.  prev_stats8 (optional):
 *       block 0 also writes the whitening coefficients of the PREVIOUS batch to prev_coef,
 *       with beta = ctl->state_in[TRLX_CTL_KL_COEF] (or kl_coef without ctl).  mom_lag = 1:
 *       ctl->global_moments are the PREVIOUS batch's all-reduced score moments, merged into
 *       RunningMoments now (NULL: none yet); not with TRLX_SCALE_RUNNING.  done_event (a
 *       hipEvent_t or NULL) is recorded by the launch's own dispatch.
 *   trlx_ppo_whiten_coef  the same coefficients as a launch of its own (ctl_state may be NULL):
 *       coef = {mean, rsqrt(var + 1e-8), beta, 0} of A = A0 - beta*Ak (modeling.py:24-34;
 *       unbiased: torch.var_mean, else the distributed biased variance).
 *   trlx_ppo_loss_rows_split  trlx_ppo_loss_rows with the advantage A0 - coef[2]*Ak whitened
 *       by coef, the mask sum at *msum (stats8 + 6), and this batch's rewards
 *       (-beta*rew_kl + rew_score) and returns (A + old_values, r_dtype) written here.  The
 *       loss tail takes stats8 + 3 as its `stats` (it reads Σ mask at stats[3]). */
int trlx_ppo_rollout_gae_split(int64_t B, int64_t T, const float* lp, const float* ref_lp, const void* values,
                               int v_dtype, const float* scores, const int64_t* lengths, const int64_t* mask,
                               const trlx_score_ctl* ctl, float kl_coef, double gamma, double lam, float* adv0,
                               float* adv_kl, float* rew_kl, float* rew_score, double* stats8,
                               const double* prev_stats8, float* prev_coef, int prev_unbiased, int mom_lag,
                               void* workspace, void* stream, void* done_event);
/* RunningMoments merge of an all-reduced {Σx, Σx², n} score record into the controller
 * state (state_out may alias state_in): the last merge of a pipelined sequence whose GAE
 * launches merged each batch's moments one batch late (mom_lag = 1 above: the scores are not
 * scaled by the running std, so the merge can wait for the moments' all-reduce to hide
 * behind the next batch's rows). */
int trlx_score_moments_merge(const double* state_in, double* state_out, const double* moments, void* stream);
int trlx_ppo_whiten_coef(const double* stats8, int unbiased, const double* ctl_state, float kl_coef, float* coef,
                         void* stream);
int trlx_ppo_loss_rows_split(const void* logits, int dtype, int64_t B, int64_t T, int64_t V, int64_t sb,
                             int64_t st, const int64_t* labels, int64_t lb, int64_t lt, const void* old_lp,
                             int old_dtype, const float* adv0, const float* adv_kl, const float* rew_kl,
                             const float* rew_score, const float* coef, const double* msum, const int64_t* mask,
                             const void* values, int v_dtype, const void* old_values, int ov_dtype, float* rewards,
                             void* returns, int r_dtype, float cliprange, float cliprange_value, float vf_coef,
                             float* lp_out, void* dx, int64_t dsb, int64_t dst, float* dvalues, void* workspace,
                             void* stream);
/* The arguments of trlx_ppo_rollout_gae_split (without the previous-batch coefficients and
 * the done event) as one POD, for a GAE folded into another launch. */
typedef struct {
    int64_t B, T;
    const float* lp;
    const float* ref_lp;
    const void* values;
    int v_dtype;
    const float* scores;              /* [B] or NULL */
    const int64_t* lengths;           /* [B] or NULL */
    const int64_t* mask;              /* [B,T] or NULL */
    const trlx_score_ctl* ctl;        /* or NULL */
    float kl_coef;
    double gamma, lam;                /* doubles: see trlx_gae_scan */
    float* adv0;
    float* adv_kl;
    float* rew_kl;
    float* rew_score;
    double* stats8;
    int mom_lag;
    void* workspace;                  /* trlx_ppo_workspace_bytes(B, T) */
} trlx_gae_split_args;
/* trlx_ppo_loss_rows_split of batch k whose rows derive the whitening coefficients
 * themselves — coef = {mean, rsqrt(var + 1e-8), beta, 0} of A = A0 - beta*Ak from the
 * (all-reduced) split record stats8, beta = ctl_state[TRLX_CTL_KL_COEF] or kl_coef when
 * ctl_state is NULL (modeling.py:24-34) — so no coefficient launch sits between the record's
 * all-reduce and the rows; row 0 stores them to `coef` for a later trlx_ppo_loss_rows_split on
 * the same experience (the ppo_epochs pattern: beta stays the experience's).  `gae` (or NULL):
 * the split GAE of the NEXT batch (ppo_orchestrator.py:163-167, ppo_models.py:121-139) runs as
 * this launch's first workgroups — nothing in it depends on these rows, so the pipelined DP
 * schedule needs no GAE launch of its own.  It must write the other split buffer set; with a
 * ctl it reads ctl->state_in and writes ctl->state_out, and ctl_state here must not be the
 * state_out.  done_event (a hipEvent_t or NULL) is recorded by the launch's own dispatch. */
int trlx_ppo_loss_rows_split_gae(const void* logits, int dtype, int64_t B, int64_t T, int64_t V, int64_t sb,
                                 int64_t st, const int64_t* labels, int64_t lb, int64_t lt, const void* old_lp,
                                 int old_dtype, const float* adv0, const float* adv_kl, const float* rew_kl,
                                 const float* rew_score, const double* stats8, int unbiased, const double* ctl_state,
                                 float kl_coef, float* coef, const double* msum, const int64_t* mask,
                                 const void* values, int v_dtype, const void* old_values, int ov_dtype,
                                 float* rewards, void* returns, int r_dtype, float cliprange, float cliprange_value,
                                 float vf_coef, float* lp_out, void* dx, int64_t dsb, int64_t dst, float* dvalues,
                                 void* workspace, const trlx_gae_split_args* gae, void* stream, void* done_event);

/* ---------------------------------------------------------------- RCCL stats all-reduce helper
 * SURVEY §8b "Collectives" — replaces the two dist.all_reduce calls of
 * get_global_statistics (trlx/utils/modeling.py:13-14, 18-19) on the hot path: ONE
 * communicator per process, SUM of a small fp64 vector ({Σx, Σx², n[, Σmask]} or the score
 * moments) enqueued on the caller's HIP stream — no side stream, no system-scope event join
 * (each of ProcessGroupNCCL's costs ~20 us of compute-queue idle on MI355X).
 *   trlx_comm_load      dlopen the RCCL the process already uses (PyTorch's librccl.so path)
 *   trlx_comm_unique_id rank 0: ncclGetUniqueId into a trlx_comm_unique_id_bytes() buffer,
 *                       which the caller broadcasts (the bindings use torch.distributed)
 *   trlx_comm_init      every rank, collectively: ncclCommInitRank on the current HIP device
 *   trlx_comm_allreduce_sum_f64   in-place SUM of buf[0:n] on `stream`
 *   trlx_comm_destroy   ncclCommDestroy */
int trlx_comm_load(const char* librccl_path);
int64_t trlx_comm_unique_id_bytes(void);
int trlx_comm_unique_id(void* id_out, int64_t nbytes);
int trlx_comm_init(void** comm_out, const void* id, int64_t nbytes, int nranks, int rank);
int trlx_comm_allreduce_sum_f64(void* comm, double* buf, int64_t n, void* stream);
int trlx_comm_destroy(void* comm);

/* ---------------------------------------------------------------- autograd plumbing
 * out[i] = x[i] * (*scale) for i < n (scale: device fp32 scalar, e.g. a backward's
 * grad_output).  In place (out == x) it is skipped entirely when *scale == 1. */
int trlx_scale_by(const void* x, void* out, int dtype, int64_t n, const float* scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRLX_T5_AMD_H */
