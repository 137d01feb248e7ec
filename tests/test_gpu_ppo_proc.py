"""The processing sampling step (csrc/ppo_sample.hip k_ppo_sample<.., true, true>,
trlx_ppo_sample_proc, sampling.ppo_sample_step(processors=, prefix=), PPOLogitsProcessors,
PPOConfig.sample_step with the processor keys in gen_kwargs).

  1  the processed row, bit for bit: smallest kept logit and kept count with nothing filtered,
     and the greedy token / its logit, on every reachable launch-table entry of both dtypes
  2  the kept set and the draw under top-k / top-p; banned tokens are never drawn
  3  log-probs of the unmodified rows, plain and recording route, forced token at the row minimum
  4  forced steps with and without a recorder
  5  everything off: bit-identical to trlx_ppo_sample / trlx_ppo_sample_record
  6  prefix tokens outside [0, V)
  7  the entry's refusals, each before any launch
  8  a 6-step decode loop through PPOConfig against torch edits of the slab

Expected values come from ppo_proc_checks.processed (fp32 torch on the CPU, pinned to
transformers' classes by tests/test_ppo_proc_cpu.py) on the inputs as the kernel sees them.
The launch table has nine entries; two (fp32 16 x 512, bf16 8 x 512) cover no vocabulary that an
earlier entry does not take, so seven can run (ppo_record_checks.SHAPES)."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import ppo_proc_checks as C
from ppo_record_checks import ATOL, RTOL, SHAPES, dname, ref_want
from ppo_sample_checks import (BF16, DEV, F32, GUARD, LOGIT_POISON, OUT_DTYPES, check_draw_and_logprob, line_ld,
                               oracle_keep, place, run_abi, select)

pytestmark = pytest.mark.gpu
NEG = float("-inf")
SHAPE_IDS = [f"{dname(d)}-N{e[0]}x{e[1]}-V{v}" for d, e, v in SHAPES]
WORDS = [[7], [3, 9], [1, 2, 3]]


def bits(t):
    return t.contiguous().view(torch.int32)


def rows(B, V, dtype, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, V, generator=g)).to(dtype)


def prefix_for(x, n, seed):
    """int64 [B, n] from a pool of 14 tokens per row: the row's argmax and argmin (so the penalty
    moves the largest and the smallest logit), the bad words' tokens, 0 and V - 1, and random
    ones; rows 0 / 1 end with [1, 2] / [3], the bad words' own prefixes; from n = 10 on row 2
    has period 5, so that every n-gram in it repeats."""
    B, V = x.shape
    g = torch.Generator().manual_seed(seed)
    xf = x.float()
    pool = torch.cat([xf.argmax(-1, keepdim=True), xf.argmin(-1, keepdim=True),
                      torch.tensor([[0, V - 1, 1, 2, 3, 9]]).expand(B, -1), torch.randint(0, V, (B, 6), generator=g)], 1)
    p = pool.gather(1, torch.randint(0, pool.shape[1], (B, n), generator=g))
    if n >= 2:
        p[0, -2:] = torch.tensor([1, 2])
    if n >= 1:
        p[1 % B, -1] = 3
    if n >= 10:
        p[2 % B] = torch.arange(n) % 5 + 20
    return p


def guarded(B):
    bufs = [torch.full((B + 16,), GUARD, dtype=d, device=DEV) for d in OUT_DTYPES]
    return bufs, [b[8:8 + B] for b in bufs]


def guards_hold(bufs, B, untouched=False):
    for b in bufs:
        assert bool((b[:8] == GUARD).all()) and bool((b[8 + B:] == GUARD).all()), "a write outside the outputs"
        if untouched:
            assert bool((b == GUARD).all()), "a refused call wrote an output"


def proc_args(lg, u, out, *, T=1.0, top_k=0, top_p=1.0, min_keep=1, cur_len=0, min_length=0, eos=None, pad=None,
              unfinished=None, rp=1.0, g=0, forced=-1, seg0=None, n0=None, seg1=None, n1=None, words=None,
              rec=None, ref=None, score_finished=False):
    """The entry's struct from device tensors as they are (strides from stride(0)).  words: a
    PPOLogitsProcessors whose table is passed; rec / ref: a PPORolloutRecorder and reference rows."""
    B, V = lg.shape
    a = _lib.PpoSampleProcArgs()
    a.logits, a.ld_logits, a.B, a.V, a.dtype = lg.data_ptr(), lg.stride(0) if B > 1 else V, B, V, _lib.dtype_code(lg)
    a.top_k, a.temperature, a.top_p, a.min_tokens_to_keep = int(top_k), float(T), float(top_p), int(min_keep)
    a.cur_len, a.min_length = int(cur_len), int(min_length)
    a.eos_token_id, a.pad_token_id = -1 if eos is None else int(eos), -1 if pad is None else int(pad)
    a.u, a.unfinished = u.data_ptr(), _lib.ptr(unfinished)
    a.out_ids, a.out_logprobs, a.out_min_kept, a.out_kept_count = [o.data_ptr() for o in out]
    a.repetition_penalty, a.no_repeat_ngram_size, a.forced_token_id = float(rp), int(g), int(forced)
    for k, (seg, n) in enumerate(((seg0, n0), (seg1, n1))):
        if seg is not None:
            setattr(a, f"prefix{k}", seg.data_ptr())
            setattr(a, f"prefix{k}_ld", seg.stride(0))
            setattr(a, f"prefix{k}_len", seg.shape[1] if n is None else n)
    if words is not None:
        a.bad_words, a.bad_words_offsets = words.bad_tokens.data_ptr(), words.bad_offsets.data_ptr()
        a.bad_words_host, a.bad_words_offsets_host = words._host_tokens.data_ptr(), words._host_offsets.data_ptr()
        a.n_bad_words = words.n_bad_words
    if rec is not None:
        a.ref_logits, a.ld_ref, a.ref_dtype, a.t, a.T = ref.data_ptr(), ref.stride(0), _lib.dtype_code(ref), rec.t, rec.T
        a.tokens, a.ld_tokens = rec.tokens.data_ptr(), rec.tokens.stride(0)
        a.logprobs, a.ld_logprobs = rec.logprobs.data_ptr(), rec.logprobs.stride(0)
        a.ref_logprobs, a.ld_ref_logprobs = rec.ref_logprobs.data_ptr(), rec.ref_logprobs.stride(0)
        a.ld_values, a.lengths, a.score_finished = rec.values.stride(0), rec.lengths.data_ptr(), int(score_finished)
    return a


def proc_abi(lg, u, **kw):
    """trlx_ppo_sample_proc into guard-filled outputs; synchronises; the four outputs on the CPU."""
    B = lg.shape[0]
    bufs, out = guarded(B)
    a = proc_args(lg, u, out, **kw)
    _lib.call("trlx_ppo_sample_proc", ctypes.byref(a), _lib.stream_of(lg))
    torch.cuda.synchronize()
    guards_hold(bufs, B)
    return tuple(o.cpu() for o in out)


def step(lg, u, pr, prefix, **kw):
    """ppo_sample_step(processors=, prefix=) -> (ids, lp, min_kept, kept_count) on the CPU."""
    B = lg.shape[0]
    out = tuple(torch.empty(B, dtype=d, device=DEV) for d in OUT_DTYPES)
    P.ppo_sample_step(lg, u=u, out=out, processors=pr, prefix=None if prefix is None else prefix.to(DEV), **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu() for o in out)


def check_processed_row(lg, u, pr, prefix, want, **kw):
    """Nothing filtered: smallest kept logit / kept count of the processed row; greedy: the token
    is its argmax and the smallest kept logit its maximum — all bit for bit."""
    mn, cnt = C.finite_min_and_count(want)
    ids, _, gmin, gcnt = step(lg, u, pr, prefix, **kw)
    assert torch.equal(bits(gmin), bits(mn)), (gmin, mn)
    assert torch.equal(gcnt, cnt), (gcnt, cnt)
    assert bool(torch.isfinite(want[torch.arange(want.shape[0]), ids]).all()), "a banned token was drawn"
    top = want.max(-1)
    if bool((want == top.values[:, None]).sum(-1).eq(1).all()):   # a unique maximum
        ids, _, gmin, gcnt = step(lg, u, pr, prefix, top_k=1, **kw)
        assert torch.equal(ids, top.indices) and torch.equal(bits(gmin), bits(top.values)) and bool((gcnt == 1).all())


# ------------------------------------------------------------------ 1. the processed row
@pytest.mark.parametrize("dtype,entry,V", SHAPES, ids=SHAPE_IDS)
def test_processed_row_bit_exact_on_every_launch_entry(dtype, entry, V):
    """Each processor alone, all together, prefix lengths 0 and 1, g - 2 / g - 1 / g, and a
    prefix longer than the entry's thread count."""
    assert select(V, dtype) == entry
    B = 3
    x = rows(B, V, dtype, 7 + V)
    lg = x.to(DEV)
    u = torch.tensor([0.2, 0.5, 0.9], device=DEV)
    every = dict(rp=1.3, g=3, bad_words=WORDS)
    cases = [(dict(rp=1.3), 9), (dict(rp=0.8), 9), (dict(g=1), 9), (dict(g=2), 9), (dict(bad_words=WORDS), 9),
             (dict(g=3), 1), (dict(g=3), 2), (dict(g=3), 3), (dict(g=3), 40),
             (every, 0), (every, 1), (every, 9), (dict(rp=0.8, g=2, bad_words=WORDS), 1100)]
    assert 1100 > entry[1]
    changed = 0
    for kw, n in cases:
        prefix = prefix_for(x, n, 100 + n)
        if n >= 40:
            assert bool((C.processed(x.float().clamp(min=-9), prefix, g=3)[2] == NEG).any())
        pr = P.PPOLogitsProcessors(V, DEV, repetition_penalty=kw.get("rp", 1.0),
                                   no_repeat_ngram_size=kw.get("g", 0), bad_words_ids=kw.get("bad_words"))
        want = C.processed(x, prefix, **kw)
        changed += int((want != x.float()).sum())
        check_processed_row(lg, u, pr, prefix, want)
    assert changed > 0


@pytest.mark.parametrize("dtype,V", [(F32, 37), (F32, 4035), (BF16, 50257)], ids=["f32-V37", "f32-V4035", "bf16-V50257"])
def test_prefix_split_across_the_two_segments_at_every_cut(dtype, V):
    """A length-5 prefix as segment 0 of c tokens and segment 1 of 5 - c, c = 0 .. 5, the two
    with different row strides: one result, the oracle's."""
    B = 3
    x = rows(B, V, dtype, 3)
    lg, u = x.to(DEV), torch.tensor([0.1, 0.6, 0.95], device=DEV)
    prefix = prefix_for(x, 5, 11)
    prefix[2] = torch.tensor([4, 6, 4, 6, 4])      # the 3-gram's match straddles every cut
    pr = P.PPOLogitsProcessors(V, DEV, bad_words_ids=WORDS)
    want = C.processed(x, prefix, rp=1.3, g=3, bad_words=WORDS)
    assert want[2, 6] == NEG and want[0, 3] == NEG
    mn, cnt = C.finite_min_and_count(want)
    wide = torch.full((B, 9), V - 1, dtype=torch.int64)
    wide[:, :5] = prefix
    wide = wide.to(DEV)
    for c in range(6):
        seg1 = prefix[:, c:].contiguous().to(DEV) if c < 5 else None
        got = proc_abi(lg, u, rp=1.3, g=3, words=pr, seg0=wide if c else None, n0=c, seg1=seg1)
        assert torch.equal(bits(got[2]), bits(mn)) and torch.equal(got[3], cnt), c


# ------------------------------------------------------------------ 2. kept set and draw
@pytest.mark.parametrize("filt", [dict(top_k=50), dict(top_p=0.9), dict(top_k=50, top_p=0.9)],
                         ids=["topk", "topp", "topk-topp"])
@pytest.mark.parametrize("dtype,V", [(F32, 4035), (BF16, 32128), (BF16, 50257)], ids=["f32-V4035", "bf16-V32128",
                                                                                   "bf16-V50257"])
def test_kept_set_and_draw_after_the_processors(dtype, V, filt):
    B, T, eos = 4, 0.7, 5
    x = rows(B, V, dtype, 21)
    lg = x.to(DEV)
    u = torch.tensor([0.03, 0.41, 0.77, 0.999], device=DEV)
    prefix = prefix_for(x, 9, 5)
    pr = P.PPOLogitsProcessors(V, DEV, repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=WORDS)
    want = C.processed(x, prefix, rp=1.3, g=2, bad_words=WORDS, eos=eos)
    ids, lp, mn, cnt = step(lg, u, pr, prefix, temperature=T, cur_len=2, min_length=4, eos_token_id=eos, **filt)
    keep, w = oracle_keep(want.double(), T, filt.get("top_k", 0), filt.get("top_p", 1.0))
    check_draw_and_logprob(x.float(), want.double(), keep, w, ids, lp, u.cpu())
    assert torch.equal(cnt, keep.sum(-1).to(torch.int32))
    assert torch.equal(bits(mn), bits(torch.where(keep, want, torch.full_like(want, float("inf"))).min(-1).values))


@pytest.mark.parametrize("uval", [0.0, 1.0 - 2.0 ** -24], ids=["u0", "u-below-1"])
@pytest.mark.parametrize("dtype,V", [(F32, 37), (BF16, 8071)], ids=["f32-V37", "bf16-V8071"])
def test_banned_tokens_are_never_drawn(dtype, V, uval):
    """The largest logit of every row is banned (n-gram, a one-token and a two-token bad word),
    and so are token 0 and token V - 1, where u = 0 and u just under 1 land."""
    B = 3
    x = rows(B, V, dtype, 2).float()
    x[:, 0], x[:, V - 1] = 1.0, 1.0
    x[:, 1], x[:, V - 2] = 6.0, 6.0
    x[0, 11], x[1, 12], x[2, 13] = 30.0, 30.0, 30.0
    x = x.to(dtype)
    prefix = torch.tensor([[4, 11, 6, 4], [8, 8, 8, 10], [8, 6, 8, 6]])
    words = [[12], [6, 13], [0], [V - 1]]        # row 0: 2-gram (4, 11) repeats; row 1: [12]; row 2: ends with 6
    want = C.processed(x, prefix, g=2, bad_words=words)
    assert want[0, 11] == NEG and want[1, 12] == NEG and want[2, 13] == NEG and want[0, 13] != NEG
    pr = P.PPOLogitsProcessors(V, DEV, no_repeat_ngram_size=2, bad_words_ids=words)
    u = torch.full((B,), uval, device=DEV)
    ids, lp, mn, cnt = step(x.to(DEV), u, pr, prefix)
    keep, w = oracle_keep(want.double(), 1.0, 0, 1.0)
    check_draw_and_logprob(x.float(), want.double(), keep, w, ids, lp, u.cpu())
    assert bool((ids != 0).all()) and bool((ids != V - 1).all())
    assert ids.tolist() == ([1] * B if uval == 0.0 else [V - 2] * B)


# ------------------------------------------------------------------ 3. log-probs of the unmodified rows
@pytest.mark.parametrize("dtype,entry,V", SHAPES, ids=SHAPE_IDS)
def test_logprobs_are_those_of_the_unmodified_rows(dtype, entry, V):
    """Greedy on the processed row, whose argmax differs from the unedited row's (its largest
    logit is banned, the runner-up penalised): lp and ref_lp are fp64 log_softmax of the unedited
    rows at the token, on the plain and the recording route; then a forced token whose unedited
    logit is the row minimum."""
    B = 3
    x = rows(B, V, dtype, 31 + V).float()
    ref = rows(B, V, dtype, 32 + V, scale=4.0)
    spots = torch.tensor([[0, V - 1, V // 2], [V // 3, 1, V - 2], [V - 1, V // 2 + 1, 0]])
    x[torch.arange(B)[:, None], spots] = torch.tensor([24.0, 22.0, 20.0])   # 24 / 1.3 < 20: the third wins
    x = x.to(dtype)
    order = x.float().argsort(-1, descending=True)
    prefix = torch.stack([order[:, 0], order[:, 1], order[:, 0]], 1)    # bigram (top, runner-up) then top again
    want = C.processed(x, prefix, rp=1.3, g=2)
    assert bool((want[torch.arange(B), order[:, 1]] == NEG).all())
    tok = want.argmax(-1)
    assert torch.equal(tok, spots[:, 2]) and torch.equal(order[:, :2], spots[:, :2])
    pr = P.PPOLogitsProcessors(V, DEV, repetition_penalty=1.3, no_repeat_ngram_size=2)
    lg, rf, u = x.to(DEV), ref.to(DEV), torch.full((B,), 0.5, device=DEV)
    ids, lp, _, _ = step(lg, u, pr, prefix, top_k=1)
    assert torch.equal(ids, tok)
    torch.testing.assert_close(lp.double(), ref_want(x, ids), rtol=RTOL, atol=ATOL)
    rec = P.PPORolloutRecorder(B, 2, DEV, 0, None)
    ids2, lp2, _, _ = step(lg, u, pr, prefix, top_k=1, ref_logits=rf, recorder=rec)
    assert torch.equal(ids2, tok) and torch.equal(lp2, lp) and rec.t == 1
    assert torch.equal(rec.tokens[:, 0].cpu(), tok) and torch.equal(rec.logprobs[:, 0].cpu(), lp)
    torch.testing.assert_close(rec.ref_logprobs[:, 0].cpu().double(), ref_want(ref, ids), rtol=RTOL, atol=ATOL)
    # forced: the unedited row's minimum, on both routes (the recorder's column 0 joins the prefix)
    low = int(x[0].float().argmin())
    x2 = x.clone()
    x2[:, low] = x.float().min() - 1.0
    prf = P.PPOLogitsProcessors(V, DEV, repetition_penalty=1.3, forced_bos_token_id=low)
    ids3, lp3, mn3, cnt3 = step(x2.to(DEV), u, prf, prefix[:, :1], cur_len=1)
    assert ids3.tolist() == [low] * B and mn3.tolist() == [0.0] * B and cnt3.tolist() == [1] * B
    torch.testing.assert_close(lp3.double(), ref_want(x2, ids3), rtol=RTOL, atol=ATOL)
    prf2 = P.PPOLogitsProcessors(V, DEV, forced_eos_token_id=low, max_length=3)
    ids4, lp4, _, _ = step(x2.to(DEV), u, prf2, prefix[:, :1], cur_len=2, ref_logits=rf, recorder=rec)
    assert ids4.tolist() == [low] * B and torch.equal(bits(lp4), bits(lp3))
    torch.testing.assert_close(rec.ref_logprobs[:, 1].cpu().double(), ref_want(ref, ids4), rtol=RTOL, atol=ATOL)
    assert torch.equal(rec.logprobs[:, 1].cpu(), lp4) and rec.tokens[:, 1].tolist() == [low] * B


# ------------------------------------------------------------------ 4. forced steps
@pytest.mark.parametrize("recording", [False, True], ids=["plain", "recorder"])
@pytest.mark.parametrize("which", ["bos", "eos"])
@pytest.mark.parametrize("dtype,V", [(F32, 37), (BF16, 32128)], ids=["f32-V37", "bf16-V32128"])
def test_forced_steps(dtype, V, which, recording):
    """cur_len == 1 forces bos, cur_len == max_length - 1 forces eos: the forced id on live rows,
    pad on the finished one, kept count 1; a forced eos finishes the rows and sets lengths."""
    B, T, pad, eos, bos, max_length = 4, 8, 0, 1, 5, 7
    x, ref = rows(B, V, dtype, 41), rows(B, V, dtype, 42)
    pr = P.PPOLogitsProcessors(V, DEV, repetition_penalty=1.2, no_repeat_ngram_size=2, forced_bos_token_id=bos,
                               forced_eos_token_id=eos, max_length=max_length, eos_token_id=eos)
    cur_len = 1 if which == "bos" else max_length - 1
    tok = bos if which == "bos" else eos
    unf = torch.tensor([1, 1, 0, 1], dtype=torch.int64, device=DEV)
    u = torch.tensor([0.0, 0.5, 0.5, 0.999], device=DEV)
    prefix = torch.zeros(B, cur_len, dtype=torch.int64)
    kw = dict(cur_len=cur_len, eos_token_id=eos, pad_token_id=pad, top_k=20, temperature=0.8, min_length=3)
    rec = None
    if recording:
        rec = P.PPORolloutRecorder(B, T, DEV, pad, eos)
        rec.unfinished.copy_(unf)
        rec.t = t = 2
        ids, lp, mn, cnt = step(x.to(DEV), u, pr, prefix, ref_logits=ref.to(DEV), recorder=rec, **kw)
        unf = rec.unfinished
    else:
        ids, lp, mn, cnt = step(x.to(DEV), u, pr, prefix, unfinished=unf, **kw)
    assert ids.tolist() == [tok, tok, pad, tok] and cnt.tolist() == [1, 1, 0, 1] and mn.tolist() == [0.0] * B
    live = torch.tensor([True, True, False, True])
    torch.testing.assert_close(lp.double()[live], ref_want(x, ids)[live], rtol=RTOL, atol=ATOL)
    assert float(lp[2]) == 0.0
    assert unf.tolist() == ([1, 1, 0, 1] if which == "bos" else [0, 0, 0, 0])
    if recording:
        assert rec.t == t + 1 and torch.equal(rec.tokens[:, t].cpu(), ids) and torch.equal(rec.logprobs[:, t].cpu(), lp)
        torch.testing.assert_close(rec.ref_logprobs[:, t].cpu().double()[live], ref_want(ref, ids)[live], rtol=RTOL,
                                   atol=ATOL)
        assert rec.lengths.tolist() == ([T] * B if which == "bos" else [t + 1, t + 1, T, t + 1])
    # one step off the forced position nothing is forced
    ids, _, _, cnt = step(x.to(DEV), u, pr, torch.zeros(B, cur_len + 1, dtype=torch.int64), **dict(kw, cur_len=cur_len + 1))
    assert bool((cnt >= 20).all()) and bool((cnt < V).all())   # (ties at the threshold are kept)


# ------------------------------------------------------------------ 5. everything off
@pytest.mark.parametrize("dtype,entry,V", SHAPES, ids=SHAPE_IDS)
def test_everything_off_is_the_plain_and_the_recording_step(dtype, entry, V):
    """No processor, no forced token (a prefix is still passed): the four outputs, unfinished and
    the recorded columns are bit-identical to trlx_ppo_sample / trlx_ppo_sample_record."""
    B, T, eos, pad = 4, 2, 5, 0
    lg, ref = rows(B, V, dtype, 11).to(DEV), rows(B, V, dtype, 12).to(DEV)
    u = torch.tensor([0.03, 0.41, 0.77, 0.999], device=DEV)
    unf0 = torch.tensor([1, 1, 0, 1], dtype=torch.int64, device=DEV)
    prefix = torch.randint(0, V, (B, 6), device=DEV)
    kw = dict(T=0.7, top_k=50, top_p=0.9, cur_len=1, min_length=3, eos=eos, pad=pad)
    ua, ub = unf0.clone(), unf0.clone()
    want = run_abi(lg, u, unfinished=ua, **kw)
    got = proc_abi(lg, u, unfinished=ub, seg0=prefix, **kw)
    for w, g in zip(want, got):
        assert torch.equal(w, g)
    assert torch.equal(ua, ub)
    ra, rb = P.PPORolloutRecorder(B, T, DEV, pad, eos), P.PPORolloutRecorder(B, T, DEV, pad, eos)
    for r in (ra, rb):
        r.unfinished.copy_(unf0)
    wkw = dict(temperature=0.7, top_k=50, top_p=0.9, cur_len=1, min_length=3, eos_token_id=eos, pad_token_id=pad)
    out = tuple(torch.empty(B, dtype=d, device=DEV) for d in OUT_DTYPES)
    P.ppo_sample_step(lg, u=u, out=out, ref_logits=ref, recorder=ra, **wkw)
    got = proc_abi(lg, u, unfinished=rb.unfinished, seg0=prefix, rec=rb, ref=ref, **kw)
    torch.cuda.synchronize()
    for w, g in zip(out, got):
        assert torch.equal(w.cpu(), g)
    for k in ("tokens", "logprobs", "ref_logprobs", "lengths", "unfinished"):
        assert torch.equal(getattr(ra, k), getattr(rb, k)), k
    for w, g in zip(want, got):    # and the recording route's policy outputs are the plain step's
        assert torch.equal(w, g)


# ------------------------------------------------------------------ 6. prefix tokens outside [0, V)
@pytest.mark.parametrize("dtype,V", [(F32, 37), (F32, 4035), (BF16, 50257)], ids=["f32-V37", "f32-V4035", "bf16-V50257"])
def test_out_of_range_prefix_tokens_are_ignored(dtype, V):
    """-1, V and 2**40 inside the prefix, the logits rows inside poison-filled slack: the result
    is the oracle's, which skips those tokens as targets, and equals the call on the prefix
    with those positions replaced by an in-range token that is no target either (the row's own
    banned token); the output guards hold."""
    B = 3
    x = rows(B, V, dtype, 51)
    lg = place(x, 16 + 2 * x.element_size(), line_ld(V, dtype), fill=LOGIT_POISON)
    u = torch.tensor([0.2, 0.5, 0.9], device=DEV)
    prefix = prefix_for(x, 12, 9)
    prefix[:, 2], prefix[:, 5], prefix[:, 7] = -1, V, 2 ** 40
    prefix[2, 8:] = torch.tensor([6, V, 6, 6])          # the 2-gram (6, V) repeats: its ban has no target
    pr = P.PPOLogitsProcessors(V, DEV, bad_words_ids=WORDS)
    kw = dict(rp=1.3, g=2, bad_words=WORDS)
    want = C.processed(x, prefix, **kw)
    got = proc_abi(lg, u, rp=1.3, g=2, words=pr, seg0=prefix.to(DEV))
    mn, cnt = C.finite_min_and_count(want)
    assert torch.equal(bits(got[2]), bits(mn)) and torch.equal(got[3], cnt)
    assert bool(torch.isfinite(want[torch.arange(B), got[0]]).all())
    top = proc_abi(lg, u, rp=1.3, g=2, words=pr, seg0=prefix.to(DEV), top_k=1)
    assert torch.equal(top[0], want.argmax(-1)) and torch.equal(bits(top[2]), bits(want.max(-1).values))
    skipped = prefix.clone()
    skipped[(prefix < 0) | (prefix >= V)] = 7             # [7] is a bad word: banned with or without it
    want2 = C.processed(x, skipped, **kw)
    assert torch.equal(bits(want2), bits(want))
    assert torch.equal(lg.cpu(), x)


# ------------------------------------------------------------------ 7. the entry's refusals
def test_entry_refusals_come_before_any_launch():
    B, V = 3, 37
    lg, u = rows(B, V, F32, 1).to(DEV), torch.rand(B, device=DEV)
    seg = torch.zeros(B, 4, dtype=torch.int64, device=DEV)
    ok_words = P.PPOLogitsProcessors(V, DEV, bad_words_ids=WORDS)

    def table(tokens, offsets):
        w = P.PPOLogitsProcessors(V, DEV, bad_words_ids=WORDS)
        w._host_tokens, w._host_offsets = torch.tensor(tokens), torch.tensor(offsets)
        w.bad_tokens, w.bad_offsets, w.n_bad_words = w._host_tokens.to(DEV), w._host_offsets.to(DEV), len(offsets) - 1
        return w

    ARG, SHAPE = 5, 1
    bad = [(dict(rp=0.0), ARG), (dict(rp=-1.5), ARG), (dict(g=-1), ARG), (dict(forced=V), ARG), (dict(forced=-2), ARG),
           (dict(words=table([7, V, 9], [0, 1, 3])), ARG), (dict(words=table([7, -1, 9], [0, 1, 3])), ARG),
           (dict(words=table([7, 3, 9], [0, 2, 1, 3])), ARG), (dict(words=table([7, 3, 9], [0, 1, 1, 3])), ARG),
           (dict(words=table([7, 3, 9], [1, 2, 3])), ARG),
           (dict(seg0=seg, n0=5), SHAPE), (dict(seg1=seg, n1=5), SHAPE), (dict(seg0=seg, n0=-1), SHAPE)]
    lib = _lib.load()
    for kw, code in bad:
        bufs, out = guarded(B)
        a = proc_args(lg, u, out, **dict(dict(rp=1.3, g=2, words=ok_words, seg0=seg), **kw))
        assert lib.trlx_ppo_sample_proc(ctypes.byref(a), _lib.stream_of(lg)) == code, kw
        torch.cuda.synchronize()
        guards_hold(bufs, B, untouched=True)
    for k in ("prefix0", "prefix1"):     # n > 0 and a NULL pointer
        bufs, out = guarded(B)
        a = proc_args(lg, u, out, rp=1.3, seg0=seg, seg1=seg)
        setattr(a, k, None)
        assert lib.trlx_ppo_sample_proc(ctypes.byref(a), _lib.stream_of(lg)) == ARG, k
        torch.cuda.synchronize()
        guards_hold(bufs, B, untouched=True)
    bufs, out = guarded(B)               # a missing host mirror
    a = proc_args(lg, u, out, words=ok_words)
    a.bad_words_host = None
    assert lib.trlx_ppo_sample_proc(ctypes.byref(a), _lib.stream_of(lg)) == ARG
    assert lib.trlx_ppo_sample_proc(None, _lib.stream_of(lg)) == ARG
    rec = P.PPORolloutRecorder(B, 2, DEV, 0, None)      # the record block's own checks still hold
    a = proc_args(lg, u, out, rp=1.3, seg0=seg, rec=rec, ref=lg)
    a.t = 2
    assert lib.trlx_ppo_sample_proc(ctypes.byref(a), _lib.stream_of(lg)) == SHAPE
    torch.cuda.synchronize()
    guards_hold(bufs, B, untouched=True)
    assert bool((rec.tokens == 0).all())
    with pytest.raises(ValueError, match="cuda:0|cpu"):   # the wrapper: processors on another device
        P.ppo_sample_step(lg, processors=P.PPOLogitsProcessors(V, "cpu", repetition_penalty=1.2))
    got = proc_abi(lg, u, rp=1.3, g=2, words=ok_words, seg0=seg)   # and the accepted call runs
    assert bool((got[3] > 0).all())


# ------------------------------------------------------------------ 8. a decode loop through PPOConfig
def test_six_step_decode_loop_against_torch_edits_of_the_slab():
    """PPOConfig with the processor keys, a recorder and prefix = [B, 1] zeros (T5's decoder
    start) over 6 steps at V 1031, against the route a caller had before: the processors as torch
    edits of the slab, then the plain recording step at the same u.  Tokens are identical; the new
    route's recorded lp / ref_lp are those of the unedited slabs, the old route's are not."""
    B, V, T, pad, eos = 4, 1031, 6, 0, 1
    gk = {"forced_bos_token_id": 5, "repetition_penalty": 1.2, "no_repeat_ngram_size": 2, "max_length": 7,
          "forced_eos_token_id": 1, "top_k": 20, "temperature": 0.9, "eos_token_id": eos, "pad_token_id": pad}
    cfg = P.PPOConfig(gen_kwargs=gk)
    rec, old = P.PPORolloutRecorder(B, T, DEV, pad, eos), P.PPORolloutRecorder(B, T, DEV, pad, eos)
    start = torch.zeros(B, 1, dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(77)
    slabs, refs = [], []
    for t in range(T):
        x, r = rows(B, V, F32, 700 + t), rows(B, V, F32, 800 + t, scale=4.0)
        x[:, eos] = -30.0
        if t == 2:
            x[1, eos] = 60.0          # row 1 ends early: pad tokens then count in its prefix
        u = torch.rand(B, generator=g).to(DEV)
        cfg.sample_step(x.to(DEV), cur_len=1 + t, prefix=start, ref_logits=r.to(DEV), recorder=rec, u=u)
        hf_ids = torch.cat([start, old.tokens[:, :t]], 1).cpu()
        edited = C.processed(x, hf_ids, rp=1.2, g=2, forced=C.forced_id(1 + t, 5, 1, 7))
        P.ppo_sample_step(edited.to(DEV), ref_logits=r.to(DEV), recorder=old, u=u, top_k=20, temperature=0.9,
                          cur_len=1 + t)
        slabs.append(x)
        refs.append(r)
    torch.cuda.synchronize()
    assert torch.equal(rec.tokens, old.tokens) and torch.equal(rec.lengths, old.lengths)
    tok = rec.tokens.cpu()
    assert tok[:, 0].tolist() == [5] * B and tok[:, 5].tolist() == [eos, pad, eos, eos] and int(tok[1, 2]) == eos
    assert rec.lengths.tolist() == [6, 3, 6, 6] and rec.unfinished.tolist() == [0] * B
    (pr,) = cfg._processors.values()
    assert pr.vocab_size == V
    for t in range(T):
        live = torch.tensor([t < n for n in rec.lengths.tolist()])
        torch.testing.assert_close(rec.logprobs[:, t].cpu().double()[live], ref_want(slabs[t], tok[:, t])[live],
                                   rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(rec.ref_logprobs[:, t].cpu().double()[live], ref_want(refs[t], tok[:, t])[live],
                                   rtol=RTOL, atol=ATOL)
        assert bool((rec.logprobs[:, t].cpu()[~live] == 0).all())
    assert old.logprobs[:, 0].tolist() == [0.0] * B and bool((rec.logprobs[:, 0] < -1.0).all())
