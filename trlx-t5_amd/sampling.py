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
                    With `processors=` (a PPOLogitsProcessors) and `prefix=` the launch also
                    applies HF's prefix-aware processors — repetition penalty, no-repeat
                    n-gram, bad words — and the forced bos / eos token that
                    T5HeadWithValueModel.generate passes (ppo_models.py:620-622).
"""
import ctypes

import torch

from . import _lib

__all__ = ["ppo_sample_step", "PPOLogitsProcessors"]


class PPOLogitsProcessors:
    """The prefix-aware logits processors and forced tokens of HF generate (transformers 4.21,
    _get_logits_processor) for ppo_sample_step(processors=, prefix=): validated once, the ragged
    bad-word table built once on `device` (flat int64 tokens + int64 offsets, the convention of
    ILQLRolloutStorage) with a host mirror for the entry's argument checks.

      repetition_penalty     rp > 0, 1 = off: x[v] = x[v] < 0 ? x[v] * rp : x[v] / rp for prefix tokens
      no_repeat_ngram_size   g >= 0, 0 = off
      bad_words_ids          list of non-empty token lists; [eos_token_id] is dropped, as HF does
      forced_bos_token_id    the token of the step with cur_len == 1
      forced_eos_token_id    the token of the step with cur_len == max_length - 1 (needs max_length)

    `active` is False when nothing is set: the step is then the plain one."""

    def __init__(self, vocab_size, device, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None,
                 forced_bos_token_id=None, forced_eos_token_id=None, max_length=None, eos_token_id=None):
        V = self.vocab_size = int(vocab_size)
        if V < 1:
            raise ValueError("vocab_size must be >= 1")
        self.device = torch.device(device)
        self.repetition_penalty = float(repetition_penalty)
        if not self.repetition_penalty > 0.0:
            raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
        if int(no_repeat_ngram_size) != no_repeat_ngram_size or int(no_repeat_ngram_size) < 0:
            raise ValueError(f"no_repeat_ngram_size must be an integer >= 0, got {no_repeat_ngram_size}")
        self.no_repeat_ngram_size = int(no_repeat_ngram_size)

        def token(v, what):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < V:
                raise ValueError(f"{what} {v!r} is not a token in [0, {V})")
            return int(v)

        self.forced_bos_token_id = None if forced_bos_token_id is None else token(forced_bos_token_id,
                                                                                  "forced_bos_token_id")
        self.forced_eos_token_id = None if forced_eos_token_id is None else token(forced_eos_token_id,
                                                                                  "forced_eos_token_id")
        self.max_length = None if max_length is None else int(max_length)
        if self.forced_eos_token_id is not None and self.max_length is None:
            raise ValueError("forced_eos_token_id needs max_length (it is forced at cur_len == max_length - 1)")
        words = []
        if bad_words_ids is not None:
            if not isinstance(bad_words_ids, (list, tuple)) or len(bad_words_ids) == 0:
                raise ValueError("bad_words_ids must be a non-empty list of token lists")
            for w in bad_words_ids:
                if not isinstance(w, (list, tuple)) or len(w) == 0:
                    raise ValueError(f"bad_words_ids: {w!r} is not a non-empty list of tokens")
                w = [token(v, "bad word token") for v in w]
                if eos_token_id is None or w != [int(eos_token_id)]:
                    words.append(w)
        self.bad_words_ids = words
        self.n_bad_words = len(words)
        self.bad_tokens = self.bad_offsets = self._host_tokens = self._host_offsets = None
        if words:
            off = [0]
            for w in words:
                off.append(off[-1] + len(w))
            self._host_tokens = torch.tensor([v for w in words for v in w], dtype=torch.int64)
            self._host_offsets = torch.tensor(off, dtype=torch.int64)
            self.bad_tokens = self._host_tokens.to(self.device)
            self.bad_offsets = self._host_offsets.to(self.device)
        self.active = (self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0 or bool(words) or
                       self.forced_bos_token_id is not None or self.forced_eos_token_id is not None)

    def forced(self, cur_len):
        """The token forced at the step whose HF input_ids has length cur_len, or -1: bos at
        cur_len == 1, eos at cur_len == max_length - 1; eos wins when both fire."""
        if cur_len is None:
            return -1
        if self.forced_eos_token_id is not None and int(cur_len) == self.max_length - 1:
            return self.forced_eos_token_id
        if self.forced_bos_token_id is not None and int(cur_len) == 1:
            return self.forced_bos_token_id
        return -1


def ppo_sample_step(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_tokens_to_keep=1, cur_len=None,
                    min_length=0, eos_token_id=None, pad_token_id=None, unfinished=None, generator=None,
                    u=None, out=None, ref_logits=None, recorder=None, values=None, score_finished=False,
                    processors=None, prefix=None, prefix_len=None):
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
    decoder mask is all ones, stores there), also in the returned logprobs.

    processors (a PPOLogitsProcessors of this V and device): the processing step
    (trlx_ppo_sample_proc).  The row is edited in HF's order — repetition penalty, no-repeat
    n-gram, bad words, min length, then the token forced at this cur_len (processors.forced) —
    before temperature / top-k / top-p and the draw.  The processors read HF's input_ids of the
    step: `prefix` [B, L] int64 with unit column stride (its first prefix_len columns, default
    L; the decoder start id for T5, the padded prompt for GPT, or everything generated so far),
    followed, with a recorder, by the recorder's own tokens[:, :t].  logprobs and the recorded
    policy / reference log-probs stay those of the unmodified rows at the token, forced tokens
    included; min_kept_logit / kept_count describe the processed row (0 and 1 at a forced step).
    On bf16 rows the penalised logit stays fp32 (HF rounds it back to bf16).  Without
    `processors` the step is today's, through today's entries.

    A recorder built with clock= (a T5DecodeClock): the device-clock step
    (trlx_ppo_sample_proc_dev).  The column t, cur_len = clock.cur_len0 + t, the eos suppression
    below min_length, the forced token (processors' forced_bos_token_id / forced_eos_token_id /
    max_length, the rule of PPOLogitsProcessors.forced) and the prefix's second segment
    recorder.tokens[:, :t] are all taken on the device from the clock: the call is the same
    launch at every token, reads nothing of the device on the host, and can be captured
    (torch.cuda.graph).  A live step is bit-identical to the host step at that t; a step with the
    clock at or past T stores nothing.  cur_len must not be passed (ValueError); recorder.t is
    not touched (recorder.sync_t() reads it back after the rollout) and the clock is NOT
    advanced: the caller's decode step ends with clock.advance().  `u` may also be a contiguous
    float32 [T, B] table, row t being step t's uniforms: one torch.rand serves the rollout."""
    if processors is None:
        if prefix is not None or prefix_len is not None:
            raise ValueError("prefix / prefix_len are read by the processors: pass processors=")
    else:  # the checks that need no device come first
        if not isinstance(processors, PPOLogitsProcessors):
            raise ValueError("processors must be a PPOLogitsProcessors")
        if logits.dim() == 2 and processors.vocab_size != logits.shape[1]:
            raise ValueError(f"processors built for vocab size {processors.vocab_size}, logits have "
                             f"{logits.shape[1]}")
        if prefix is not None:
            if not isinstance(prefix, torch.Tensor) or prefix.dtype != torch.int64:
                raise ValueError("prefix must be an int64 tensor [B, L]")
            if prefix.dim() != 2 or prefix.shape[0] != logits.shape[0] or (prefix.shape[1] > 1 and
                                                                          prefix.stride(1) != 1):
                raise ValueError(f"prefix must be [B = {logits.shape[0]}, L] with unit column stride")
            if prefix_len is None:
                prefix_len = prefix.shape[1]
            if not 0 <= int(prefix_len) <= prefix.shape[1]:
                raise ValueError(f"prefix_len {prefix_len} outside [0, L = {prefix.shape[1]}]")
            if prefix.device != logits.device:
                raise ValueError(f"prefix on {prefix.device}, logits on {logits.device}")
        elif prefix_len is not None:
            raise ValueError("prefix_len without prefix")
        pd, ld = processors.device, logits.device
        if pd.type != ld.type or (pd.index or 0) != (ld.index or 0):
            raise ValueError(f"processors on {processors.device}, logits on {logits.device}")
    recording = ref_logits is not None or recorder is not None
    if recording and (ref_logits is None or recorder is None):
        raise ValueError("ref_logits and recorder go together (the recording step needs both)")
    clock = getattr(recorder, "clock", None) if recording else None
    if clock is not None:  # the device-clock step: nothing below may depend on the position
        if cur_len is not None:
            raise ValueError("cur_len with a clocked recorder: the kernel derives cur_len = clock.cur_len0 + t from "
                             "the device clock (a host value would be baked into a captured step); set cur_len0 on "
                             "the T5DecodeClock instead")
        if u is not None and u.dim() == 2:
            if u.dtype != torch.float32 or tuple(u.shape) != (recorder.T, logits.shape[0]) or not u.is_contiguous():
                raise ValueError(f"a u table must be contiguous float32 [T, B] = [{recorder.T}, {logits.shape[0]}] "
                                 f"(row t is step t's uniforms), got {u.dtype} {tuple(u.shape)}")
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
    u_ld = 0
    if u is None:
        u = torch.rand(B, generator=generator, device=dev, dtype=torch.float32)
    elif clock is not None and u.dim() == 2:  # the [T, B] table, checked above
        u_ld = B
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
    if processors is not None or clock is not None:
        pa = _lib.PpoSampleProcArgs()
        (pa.logits, pa.ld_logits, pa.dtype, pa.B, pa.V, pa.temperature, pa.top_k, pa.top_p, pa.min_tokens_to_keep,
         pa.cur_len, pa.min_length, pa.eos_token_id, pa.pad_token_id, pa.u, pa.out_ids, pa.out_logprobs,
         pa.out_min_kept, pa.out_kept_count, pa.unfinished) = step
        pa.repetition_penalty, pa.forced_token_id = 1.0, -1
        if processors is not None:
            pa.repetition_penalty = processors.repetition_penalty
            pa.no_repeat_ngram_size = processors.no_repeat_ngram_size
            if clock is None:
                pa.forced_token_id = processors.forced(cur_len)
        if prefix is not None and int(prefix_len) > 0:
            pa.prefix0, pa.prefix0_ld, pa.prefix0_len = prefix.data_ptr(), prefix.stride(0), int(prefix_len)
        if processors is not None and processors.n_bad_words:
            pa.bad_words, pa.bad_words_offsets = processors.bad_tokens.data_ptr(), processors.bad_offsets.data_ptr()
            pa.bad_words_host = processors._host_tokens.data_ptr()
            pa.bad_words_offsets_host = processors._host_offsets.data_ptr()
            pa.n_bad_words = processors.n_bad_words
        if recording:
            rec = recorder
            ref = ref_logits if ref_logits.stride(-1) == 1 else ref_logits.contiguous()
            if clock is not None:  # the kernel reads tokens[:, :t] with the clock's t
                pa.prefix1, pa.prefix1_ld = rec.tokens.data_ptr(), rec.tokens.stride(0)
            elif rec.t > 0:
                pa.prefix1, pa.prefix1_ld, pa.prefix1_len = rec.tokens.data_ptr(), rec.tokens.stride(0), rec.t
            pa.ref_logits, pa.ld_ref, pa.ref_dtype, pa.t, pa.T = ref.data_ptr(), ref.stride(0), _lib.dtype_code(ref), \
                (0 if clock is not None else rec.t), rec.T
            pa.tokens, pa.ld_tokens = rec.tokens.data_ptr(), rec.tokens.stride(0)
            pa.logprobs, pa.ld_logprobs = rec.logprobs.data_ptr(), rec.logprobs.stride(0)
            pa.ref_logprobs, pa.ld_ref_logprobs = rec.ref_logprobs.data_ptr(), rec.ref_logprobs.stride(0)
            if values is not None:
                pa.values, pa.step_values, pa.values_dtype = rec.values.data_ptr(), values.data_ptr(), \
                    _lib.dtype_code(values)
            pa.ld_values = rec.values.stride(0)
            pa.lengths = rec.lengths.data_ptr()
            pa.score_finished = int(bool(score_finished))
        if clock is not None:
            # forced bos / eos and max_length go to the entry; the kernel applies processors.forced's rule
            da = _lib.PpoSampleDevArgs(clock=clock.record.data_ptr(), forced_bos_token_id=-1, forced_eos_token_id=-1,
                                       max_length=0, u_ld=u_ld)
            if processors is not None:
                if processors.forced_bos_token_id is not None:
                    da.forced_bos_token_id = processors.forced_bos_token_id
                if processors.forced_eos_token_id is not None:
                    da.forced_eos_token_id, da.max_length = processors.forced_eos_token_id, processors.max_length
            _lib.call("trlx_ppo_sample_proc_dev", ctypes.byref(pa), ctypes.byref(da), _lib.stream_of(rows))
        else:
            _lib.call("trlx_ppo_sample_proc", ctypes.byref(pa), _lib.stream_of(rows))
            if recording:
                recorder.t += 1
    elif recording:
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
