"""trlx_t5_amd — MI355X-native (gfx950) PPO experience-and-loss hot path of trlX-T5.

Drop-in names (reference file:line in danyang-rainbow/trlx-t5):
  logprobs_from_logits, whiten, get_global_statistics, RunningMoments, flatten_dict
      trlx/utils/modeling.py
  PPOConfig (.get_advantages_and_returns, .loss, .loss_from_logits, .sample_step),
  AdaptiveKLController, FixedKLController
      trlx/model/nn/ppo_models.py
  kl_penalty_rewards, prepare_scores
      trlx/orchestrator/ppo_orchestrator.py:96-112,163-167
  ILQLConfig (.loss), ILQLBatch, ilql_sample_step (one decode step of generate)
      trlx/model/nn/ilql_models.py:52-116,296-316, trlx/data/ilql_types.py
  ILQLHeads (.forward, .forward_for_loss, .sync_target_q_heads), ilql_target_q_at_actions,
  polyak_update — the heads module: target Q at the action tokens only, fused Polyak sync
      trlx/model/nn/ilql_models.py:119-181
  FusedAdamW (.step(polyak=, max_grad_norm=)), adamw_step — opt.step() of torch.optim.AdamW as
      one launch per dtype group, fp32 masters for bf16 parameters, the ILQL target sync folded
      into the same pass (ILQLHeads.step_and_sync)   trlx/model/accelerate_base_model.py:94-106,263-265
      FusedAdamW(capturable=True, lr_schedule=, skip_nonfinite=, sync_every=), schedule_table —
      step counter, learning rate, non-finite skip and sync cadence on the device (graph capture)
      FusedAdamW(state_dtype="param") — torch's own state layout: bf16 exp_avg / exp_avg_sq for a
      bf16 parameter, every op rounded to bf16 as torch.optim.AdamW rounds it (trlx_adamw_step_ex)
  clip_grad_norm_ — the global-L2-norm clip (DeepSpeed `gradient_clipping: 1.0`), stand-alone
      or folded into the step through a device record     configs/deepspeed_configs/default_configs.yml
  ppo_sample_step — one rollout token of generate(**gen_kwargs): min length, temperature,
      top-k, top-p, the draw, unfinished / pad, and the token's policy log-prob
      trlx/orchestrator/ppo_orchestrator.py:76 (HF generate's sample path)
  PPORolloutRecorder + ppo_sample_step(ref_logits=, recorder=) — the decode loop records
      tokens, policy and reference log-probs and values per step; with
      PPOHotPath.experience_from_logprobs the teacher-forced second pass over [B, T, V] logits
      goes away      trlx/orchestrator/ppo_orchestrator.py:116-167
  PPOLogitsProcessors + ppo_sample_step(processors=, prefix=) — repetition penalty, no-repeat
      n-gram, bad words and the forced bos / eos token of generate(forced_bos_token_id=...,
      **gen_kwargs) inside the same launch; the recorded log-probs stay those of the
      unmodified rows      trlx/model/nn/ppo_models.py:620-622
  lm_head_logprobs — fused lm_head GEMM (MFMA) + logprobs, logits never in HBM
  ValueHead (.values), value_head, make_value_head — the bf16 value head make_head(n_embd, 1)
      fused: values and their gradient from hidden states, the [N, 2H] activation never
      written by the forward      trlx/model/nn/ppo_models.py:216-222,:618,:641
  t5_decode_self_attention, t5_decode_cross_attention, T5DecodeKVCache, t5_relative_bias_table —
      one decode step of a T5 decoder layer's attention over a device KV cache in one launch:
      cache append, scores, relative-position bias, encoder key mask, fp32 softmax, P·V
      (HF T5Attention between the projections and `o`, under generate)
  T5DecodeClock — the decode position t as a device record: t5_decode_self_attention(t=clock) and
      ppo_sample_step(recorder=PPORolloutRecorder(..., clock=clock)) read it on the device, so one
      captured decode step (torch.cuda.graph) replays for every token; clock.advance() ends a step
  t5_decode_embed — the decoder's input row of a decode step in one launch: the token drawn at the
      step before (read from the recorder on the device), the embedding row, layer 0's first norm;
      with `live=recorder.unfinished` both decode attentions skip the rows that have drawn eos
      (the token feedback and the finished rows of HF generate, ppo_orchestrator.py:76)
  t5_quantize_cross_kv, T5CrossKV8, t5_decode_cross_attention_kv8 — opt-in: the encoder's keys and
      values as e4m3fn bytes with a power-of-two scale per (row, head), quantised once per rollout
      in one launch, and the decode cross-attention over them: half the K / V bytes per token,
      fp32 arithmetic; lossy against the bf16 keys, exact against its own dequantised values
  t5_decode_cross_attention_grouped — the decode cross-attention of a rollout that draws G samples
      per prompt (num_return_sequences, RLOO / GRPO groups) over one copy of each prompt's keys and
      values: K / V bytes per token and K / V memory divided by G, every row bit-identical to
      t5_decode_cross_attention on the expanded tensors
  t5_decode_cross_attention_split (+ _split_plan, _split_geometry) — opt-in: the same call with the
      encoder keys of a (row, head) cut into ranges walked by workgroups of their own and merged by
      a second launch, for few rows, few live rows or long prompts; the plan is set from measurements
  t5_attention, t5_relative_bias_offsets — T5's attention over whole sequences (encoder
      self-attention, teacher-forced decoder self- and cross-attention) as one flash-attention
      launch on MFMA: bias, key mask and causal rule inside, no [Tq, S] tensor
      (HF T5Attention between the projections and `o`, ppo_orchestrator.py:119-130)
  t5_attention_train, t5_relative_bias_buckets — the same attention under autograd for the PPO
      update: MFMA backward for dq, dk, dv and the bias table, nothing of size [Tq, S] saved
  t5_ff_act, t5_ff_act_packed, T5FeedForward — the other half of a T5 layer: act(wi_0 x) * wi_1 x
      (gelu_new / silu / relu, gated or not) in one launch between the projections, fp32 arithmetic
      with one rounding, and a one-launch backward that saves u and v alone
      (HF T5DenseGatedActDense / T5DenseActDense)
  t5_rmsnorm, t5_add_rmsnorm, T5LayerNorm — T5's layer norm with the residual add of the sub-layer
      before it in one launch (h and the normed rows written, x and residual read once), fp32
      arithmetic with one rounding, and a backward of at most two launches with no atomics
      (HF T5LayerNorm, the adds of T5LayerSelfAttention / T5LayerCrossAttention / T5LayerFF)
  t5_decode_linear, T5DecodeBlockWeights, t5_decode_layer_fused — opt-in: a decode step's projections
      on a skinny MFMA kernel of our own with the RMSNorm in front, the residual add behind and the
      gated activation behind `wi` in the same launch: a decoder layer's decode step in 8 launches
      instead of 12 (HF T5Block under generate; every other projection stays hipBLASLt);
      split_rows=True spreads the rows over workgroups and live=recorder.unfinished skips the
      projections of finished rows on the device (trlx_t5_decode_linear_rows)
  PPORolloutStorage, PPORLElement, PPORLBatch
      trlx/pipeline/ppo_pipeline.py, trlx/data/ppo_types.py (device-resident store)
  ILQLRolloutStorage (.from_samples = make_experience, .collate, .create_loader), ILQLElement
      trlx/pipeline/offline_pipeline.py, trlx/orchestrator/offline_orchestrator.py:17-74,
      trlx/data/ilql_types.py (device-resident ragged store, one-launch padded collate)
  PPOHotPath — the fused device-resident experience+loss step (bench / DP shard)
  PPOControlState — RunningMoments / score scale+clip / KL controller state in HBM

All tensor math runs in hand-written HIP kernels (libtrlx_t5_amd.so, C ABI in
include/trlx_t5_amd.h).  There is no CPU fallback.
"""
from . import _lib
from .modeling import (RunningMoments, flatten_dict, get_global_statistics, grad_buffer_like,
                       logprobs_from_logits, moments, whiten)
from .ppo import (STATS_KEYS, AdaptiveKLController, FixedKLController, PPOConfig, kl_penalty_rewards,
                  prepare_scores, stats_dict)
from .lm_head import lm_head_logprobs
from .rollout_store import PPORLBatch, PPORLElement, PPORolloutRecorder, PPORolloutStorage
from .ilql import ILQL_LOSS_KEYS, ILQLBatch, ILQLConfig, ILQLHotPath, ilql_sample_step
from .ilql_heads import ILQLHeads, ilql_target_q_at_actions, make_head, polyak_update
from .optim import FusedAdamW, adamw_step, clip_grad_norm_, schedule_table
from .ilql_store import ILQLElement, ILQLRolloutStorage
from .value_head import ValueHead, value_head, value_head_splits
from .value_head import make_head as make_value_head
from .sampling import PPOLogitsProcessors, ppo_sample_step
from .t5_decode import (T5CrossKV8, T5DecodeClock, T5DecodeKVCache, t5_decode_cross_attention,
                        t5_decode_cross_attention_grouped, t5_decode_cross_attention_kv8,
                        t5_decode_cross_attention_split, t5_decode_cross_attention_split_geometry,
                        t5_decode_cross_attention_split_plan, t5_decode_embed,
                        t5_decode_self_attention, t5_quantize_cross_kv, t5_relative_bias_table)
from .t5_attention import t5_attention, t5_attention_train, t5_relative_bias_buckets, t5_relative_bias_offsets
from .t5_ff import T5FeedForward, t5_ff_act, t5_ff_act_packed
from .t5_norm import T5LayerNorm, t5_add_rmsnorm, t5_rmsnorm
from .t5_decode_linear import T5DecodeBlockWeights, t5_decode_layer_fused, t5_decode_linear
from .control import PPOControlState
from .step import PPOHotPath
from .comm import RcclComm
from .model_inputs import get_model_inputs, shift_tokens_right

__all__ = [
    "logprobs_from_logits", "whiten", "get_global_statistics", "RunningMoments", "flatten_dict", "moments",
    "grad_buffer_like", "PPOConfig", "AdaptiveKLController", "FixedKLController", "kl_penalty_rewards",
    "prepare_scores", "stats_dict", "STATS_KEYS", "PPOHotPath", "load_library",
    "ILQLConfig", "ILQLBatch", "ILQLHotPath", "ILQL_LOSS_KEYS", "ilql_sample_step", "ppo_sample_step",
    "ILQLHeads", "ilql_target_q_at_actions", "polyak_update", "make_head", "PPORolloutStorage",
    "PPORolloutRecorder", "PPOLogitsProcessors",
    "ILQLRolloutStorage", "ILQLElement",
    "PPORLElement", "PPORLBatch", "lm_head_logprobs", "PPOControlState",
    "RcclComm", "shift_tokens_right", "get_model_inputs",
    "ValueHead", "value_head", "value_head_splits", "make_value_head",
    "FusedAdamW", "adamw_step", "clip_grad_norm_", "schedule_table",
    "T5DecodeKVCache", "T5DecodeClock", "t5_decode_self_attention", "t5_decode_cross_attention", "t5_relative_bias_table",
    "t5_decode_embed", "T5CrossKV8", "t5_quantize_cross_kv", "t5_decode_cross_attention_kv8",
    "t5_decode_cross_attention_grouped", "t5_decode_cross_attention_split", "t5_decode_cross_attention_split_plan",
    "t5_decode_cross_attention_split_geometry",
    "t5_attention", "t5_relative_bias_offsets", "t5_attention_train", "t5_relative_bias_buckets",
    "t5_ff_act", "t5_ff_act_packed", "T5FeedForward",
    "t5_rmsnorm", "t5_add_rmsnorm", "T5LayerNorm",
    "t5_decode_linear", "T5DecodeBlockWeights", "t5_decode_layer_fused",
]


def load_library():
    """Load libtrlx_t5_amd.so now (raises if it is not built)."""
    return _lib.load()
