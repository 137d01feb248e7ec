"""Drop-in for the per-token sampling chain of PPO rollout generation on MI355X.

  ppo_sample_step   the logits processors and the draw that HF `generate(do_sample=True)`
                    (transformers 4.21) runs per decoded token when the orchestrator calls
                    `generate(**gen_kwargs)` (ppo_orchestrator.py:76, ppo_models.py:620-622):
                    min-length EOS suppression, temperature, top-k, top-p, softmax +
                    torch.multinomial, the unfinished / pad bookkeeping — one kernel launch
                    (csrc/ppo_sample.hip), which also returns the policy log-prob of the token.
                    With `ref_logits=` and `recorder=` the same launch scores the token under
                    the reference model's row and writes column t of the rollout's [B, T]
                    buffers (rollout_store.PPORolloutRecorder): the teacher-forced second pass
                    over [B, T, V] logits (ppo_orchestrator.py:116-161) is not needed.
"""
import torch

from . import _lib

__all__ = ["ppo_sample_step"]


def ppo_sample_step(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_tokens_to_keep=1, cur_len=None,
                    min_length=0, eos_token_id=None, pad_token_id=None, unfinished=None, generator=None,
                    u=None, out=None, ref_logits=None, recorder=None, values=None, score_finished=False):
    """One rollout token per row of logits [B, V] (the last position; fp32 or bf16, a row-strided
    view is read in place).  Returns (ids [B, 1] int64, logprobs [B] fp32).

    Order of HF's sample path: logits[eos] = -inf while cur_len < min_length; / temperature;
    top-k (0 = off; a float such as the YAMLs' 0.0 is accepted; ties at the threshold kept);
    top-p when < 1 (the token that crosses top_p stays, at least min_tokens_to_keep are kept;
    every tie at the nucleus boundary is kept, where HF keeps the one its sort placed first);
    the draw; `unfinished` (int64 [B] or [B, 1], contiguous, updated in place): a finished row
    gets pad_token_id, a live row that draws eos_token_id becomes finished.

    The draw is the inverse CDF over the kept tokens in vocab order at uniforms from `generator`
    (torch.rand on the device), or at `u` [B] when given: the distribution of
    torch.multinomial, another random stream.  logprobs = log_softmax(logits)[ids] on the
    unmodified logits (what logprobs_from_logits(logits, ids) returns).  A row with no finite
    logit left returns pad_token_id (HF raises there).

    out: optional preallocated (ids int64 [B], logprobs fp32 [B], min_kept_logit fp32 [B],
    kept_count int32 [B]) on the device — a decode loop then allocates nothing; the last two
    hold the smallest kept logit and the size of the kept set (0 for finished rows).

    ref_logits + recorder (both or neither): the recording step (trlx_ppo_sample_record).
    ref_logits [B, V] are the reference model's logits of the same step (the dtype of `logits`,
    row-strided); the token, its policy log-prob, log_softmax(ref_logits)[token] and `values`
    ([B] fp32 / bf16, optional) go to column recorder.t of the PPORolloutRecorder's buffers,
    recorder.lengths[b] becomes t + 1 where a live row draws eos, and recorder.t advances.
    The policy row takes the path of the plain step: ids, logprobs and the `out` vectors are
    bit-identical.  unfinished / pad_token_id / eos_token_id default to the recorder's.
    score_finished: False records pad, 0, 0 and value 0 after a row's eos and reads neither
    row (the ragged convention of PPOHotPath's `lengths`); True records the log-softmax of
    both rows at pad and the value as given (what the reference's teacher-forced pass, whose
    decoder mask is all ones, stores there), also in the returned logprobs."""
    recording = ref_logits is not None or recorder is not None
    if recording and (ref_logits is None or recorder is None):
        raise ValueError("ref_logits and recorder go together (the recording step needs both)")
    _lib.require_cuda(logits, unfinished, u)
    if logits.dim() != 2:
        raise ValueError("logits must be [B, V] (the last position)")
    B, V = logits.shape
    if recording:
        pad_token_id, eos_token_id, unfinished = recorder._step_inputs(logits, ref_logits, values, pad_token_id,
                                                                       eos_token_id, unfinished)
    top_k = min(int(top_k), V)
    if not float(temperature) > 0.0:
        raise ValueError("temperature must be > 0")
    if not float(top_p) > 0.0:
        raise ValueError("top_p must be > 0")
    if top_k < 0:
        raise ValueError("top_k must be >= 0 (0 disables it)")
    if int(min_tokens_to_keep) < 1:
        raise ValueError("min_tokens_to_keep must be >= 1")
    dev = logits.device
    rows = logits if logits.stride(-1) == 1 else logits.contiguous()
    unf = None
    if unfinished is not None:
        if pad_token_id is None:
            raise ValueError("unfinished needs pad_token_id (the token of a finished row)")
        unf = unfinished.reshape(B)
        if unf.dtype != torch.int64 or not unf.is_contiguous() or unf.data_ptr() != unfinished.data_ptr():
            raise ValueError("unfinished must be a contiguous int64 tensor (updated in place)")
    if u is None:
        u = torch.rand(B, generator=generator, device=dev, dtype=torch.float32)
    elif u.dtype != torch.float32 or tuple(u.shape) != (B,) or not u.is_contiguous():
        raise ValueError("u must be a contiguous float32 [B] tensor")
    if out is None:
        out = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    else:
        want = (torch.int64, torch.float32, torch.float32, torch.int32)
        if len(out) != 4 or any(t.dtype != d or tuple(t.shape) != (B,) or not t.is_contiguous() or t.device != dev
                                for t, d in zip(out, want)):
            raise ValueError("out must be (ids int64, logprobs fp32, min_kept_logit fp32, kept_count int32), "
                             "contiguous [B] tensors on the logits' device")
    ids, lp, min_kept, kept = out
    step = (rows.data_ptr(), rows.stride(0), _lib.dtype_code(rows), B, V, float(temperature),
            top_k, float(top_p), int(min_tokens_to_keep), 0 if cur_len is None else int(cur_len), int(min_length),
            -1 if eos_token_id is None else int(eos_token_id), -1 if pad_token_id is None else int(pad_token_id),
            u.data_ptr(), ids.data_ptr(), lp.data_ptr(), min_kept.data_ptr(), kept.data_ptr(), _lib.ptr(unf))
    if recording:
        rec = recorder
        ref = ref_logits if ref_logits.stride(-1) == 1 else ref_logits.contiguous()
        _lib.call("trlx_ppo_sample_record", *step, ref.data_ptr(), ref.stride(0), _lib.dtype_code(ref), rec.t, rec.T,
                  rec.tokens.data_ptr(), rec.tokens.stride(0), rec.logprobs.data_ptr(), rec.logprobs.stride(0),
                  rec.ref_logprobs.data_ptr(), rec.ref_logprobs.stride(0),
                  rec.values.data_ptr() if values is not None else None, rec.values.stride(0), _lib.ptr(values),
                  _lib.dtype_code(values) if values is not None else 0, rec.lengths.data_ptr(),
                  int(bool(score_finished)), _lib.stream_of(rows))
        rec.t += 1
    else:
        _lib.call("trlx_ppo_sample", *step, _lib.stream_of(rows))
    return ids.view(B, 1), lp
