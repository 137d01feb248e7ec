"""The decode clock on the GPU (csrc/decode_clock.hip, the device-clock instantiations of
k_t5_decode_attn and k_ppo_sample; t5_decode.T5DecodeClock, t5_decode_self_attention(t=clock),
PPORolloutRecorder(clock=), sampling.ppo_sample_step) against the host-t entries.

Every comparison is exact equality of the raw bits: the clock route and the host route execute
the same arithmetic, so no tolerance is involved.  Dead steps (the clock outside [0, T)) run
over buffers with guard margins on both sides, so that even a missing guard in the kernel would
stay inside the test's own allocations."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import decode_clock_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ERR_ARG = 5
DTYPES = (torch.bfloat16, torch.float32)


def name(dt):
    return {torch.bfloat16: "bf16", torch.float32: "fp32"}[dt]


def bits(x):
    x = x.detach().contiguous()
    if x.dtype == torch.bfloat16:
        x = x.view(torch.int16)
    elif x.dtype == torch.float32:
        x = x.view(torch.int32)
    return x.cpu()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def set_clock(clock, t):
    clock.record[_lib.CLOCK_T] = t


# ------------------------------------------------------------------ the clock itself
def test_the_clock_counts_and_overruns():
    clock = P.T5DecodeClock(3, DEV, cur_len0=2)
    assert clock.record.tolist() == [0, 3, 2, 0, 0, 0, 0, 0]
    for want_t, want_over in ((1, 0), (2, 0), (3, 0), (3, 1), (3, 2)):
        clock.advance()
        assert (clock.t, clock.overrun) == (want_t, want_over)
    clock.reset()
    assert clock.record.tolist() == [0, 3, 2, 0, 0, 0, 0, 0]
    guard = torch.full((C.CLOCK_WORDS + 2,), 5, dtype=torch.int64, device=DEV)
    stream = _lib.stream_of(guard)
    for args in ((None, 4, 1), (guard.data_ptr() + 4, 4, 1), (guard.data_ptr() + 8, 0, 1), (guard.data_ptr() + 8, 4, -1)):
        assert _lib.query("trlx_decode_clock_init", *args, stream) == ERR_ARG
    for ptr in (None, guard.data_ptr() + 4):
        assert _lib.query("trlx_decode_clock_advance", ptr, stream) == ERR_ARG
    assert guard.tolist() == [5] * (C.CLOCK_WORDS + 2)


# ------------------------------------------------------------------ 1. self-attention, clock against host t
AB, ANH, AMAX = 2, 3, 70
_ATTN = {}


def attn_case(dtype, d):
    """The inputs of one (dtype, d_kv), made once and never modified: a fused qkv projection whose
    three slices are q / k_new / v_new, the cache contents below t, the bias table."""
    if (dtype, d) not in _ATTN:
        g = torch.Generator().manual_seed(4100 + d + (1 if dtype == torch.float32 else 0))
        inner = ANH * d
        qkv = (torch.randn(AB, 3 * inner, generator=g) * d ** -0.25).to(dtype).to(DEV)
        K = (torch.randn(AB, ANH, AMAX, d, generator=g) * d ** -0.25).to(dtype).to(DEV)
        V = torch.randn(AB, ANH, AMAX, d, generator=g).to(dtype).to(DEV)
        table = P.t5_relative_bias_table(torch.randn(32, ANH, generator=g).to(DEV), AMAX)
        _ATTN[(dtype, d)] = dict(qkv=qkv, K=K, V=V, table=table, inner=inner)
    return _ATTN[(dtype, d)]


def attn_cache(c, dtype, d, t):
    """The stream's columns below t, the guard from column t on."""
    cache = P.T5DecodeKVCache(AB, ANH, d, AMAX, dtype, DEV)
    for dst, src in ((cache.k, c["K"]), (cache.v, c["V"])):
        dst.fill_(C.GUARD)
        dst[:, :, :t] = src[:, :, :t]
    return cache


@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_self_attention_with_the_clock_is_the_host_step(dtype, d):
    c = attn_case(dtype, d)
    inner = c["inner"]
    q, kn, vn = (c["qkv"][:, i * inner:(i + 1) * inner] for i in range(3))
    clock = P.T5DecodeClock(AMAX, DEV)
    for t in C.self_t(dtype, d, AMAX):
        host, dev = attn_cache(c, dtype, d, t), attn_cache(c, dtype, d, t)
        want = P.t5_decode_self_attention(q, kn, vn, host, t, c["table"])
        set_clock(clock, t)
        got = P.t5_decode_self_attention(q, kn, vn, dev, clock, c["table"])
        assert same(got, want), (t, "out")
        assert same(dev.k, host.k) and same(dev.v, host.v), (t, "cache")
        assert torch.isfinite(want.float()).all() and clock.t == t   # the step does not advance the clock


# ------------------------------------------------------------------ 2. dead steps
MARGIN = 4   # columns / elements of guard on both sides of every buffer a dead step could touch


def with_margins(shape, dtype, row):
    """A guard-filled tensor of `shape` inside a larger guard-filled allocation: MARGIN rows of
    `row` elements before and after.  Returns (whole, view)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * MARGIN * row,), C.GUARD, dtype=dtype, device=DEV)
    return whole, whole[MARGIN * row:MARGIN * row + n].view(shape)


@pytest.mark.parametrize("T,t", [(AMAX, AMAX), (AMAX, AMAX + 3), (AMAX, -1), (5, 5)], ids=str)
@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 64), (torch.float32, 128)], ids=str)
def test_a_dead_attention_step_writes_zeros_and_leaves_the_cache(dtype, d, T, t):
    assert not C.attention_live(t, T, AMAX) and -MARGIN <= t < AMAX + MARGIN
    c = attn_case(dtype, d)
    inner = c["inner"]
    k_all, k = with_margins((AB, ANH, AMAX, d), dtype, d)
    v_all, v = with_margins((AB, ANH, AMAX, d), dtype, d)
    b_all, bias = with_margins((ANH, AMAX), torch.float32, 1)
    out = torch.full((AB, inner), C.GUARD, dtype=dtype, device=DEV)
    clock = P.T5DecodeClock(T, DEV)
    set_clock(clock, t)
    q, kn, vn = (c["qkv"][:, i * inner:(i + 1) * inner] for i in range(3))
    ld = c["qkv"].stride(0)
    args = _lib.T5DecodeAttnArgs(
        q=q.data_ptr(), ldq=ld, k_new=kn.data_ptr(), ldk=ld, v_new=vn.data_ptr(), ldv=ld, k=k.data_ptr(),
        v=v.data_ptr(), bias_by_distance=bias.data_ptr(), key_mask=None, out=out.data_ptr(), B=AB, n_heads=ANH,
        d_kv=d, max_len=AMAX, t=0, dtype=_lib.dtype_code(k), mode=_lib.T5_ATTN_SELF)
    _lib.call("trlx_t5_decode_attn_dev", ctypes.byref(args), clock.record.data_ptr(), _lib.stream_of(out))
    torch.cuda.synchronize()
    assert same(out, torch.zeros_like(out))
    for whole in (k_all, v_all, b_all):
        assert same(whole, torch.full_like(whole, C.GUARD))
    assert clock.record.tolist() == [t, T, 1, 0, 0, 0, 0, 0]


SB, ST = 5, 7


def margin_recorder(clock, pad, eos):
    """A clocked recorder whose [B, T] buffers sit inside guard margins; returns (recorder, wholes)."""
    rec = P.PPORolloutRecorder(SB, ST, DEV, pad_token_id=pad, eos_token_id=eos, clock=clock)
    wholes = {}
    for field, dtype in (("tokens", torch.int64), ("logprobs", torch.float32), ("ref_logprobs", torch.float32),
                         ("values", torch.float32)):
        wholes[field], view = with_margins((SB, ST), dtype, 1)
        setattr(rec, field, view)
    for field in ("lengths", "unfinished"):
        wholes[field], view = with_margins((SB,), torch.int64, 1)
        setattr(rec, field, view)
    rec.reset()
    return rec, wholes


@pytest.mark.parametrize("T,t", [(ST, ST), (ST, ST + 3), (ST, -1)], ids=str)
@pytest.mark.parametrize("processing", (False, True), ids=("record", "proc"))
def test_a_dead_sampling_step_stores_nothing(processing, T, t):
    V, pad, eos = 517, 0, 1
    assert not C.clock_rule(t, T, 1, buffers_T=ST)["live"] and -MARGIN < t < ST + MARGIN
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(SB, V, generator=g).to(torch.bfloat16).to(DEV)
    ref = torch.randn(SB, V, generator=g).to(torch.bfloat16).to(DEV)
    values = torch.randn(SB, generator=g).to(DEV)
    clock = P.T5DecodeClock(T, DEV)
    rec, wholes = margin_recorder(clock, pad, eos)
    rec.unfinished[2] = 0
    rec.tokens.copy_(torch.randint(0, V, (SB, ST), generator=g))   # a prefix a live step would read
    # the uniforms: a leading guard row, the [T, B] table, T + 4 rows allocated behind its start
    u_all = torch.full((1 + ST + 4, SB), C.GUARD, device=DEV)
    u = u_all[1:1 + ST]
    out = (torch.full((SB,), -3, dtype=torch.int64, device=DEV), torch.full((SB,), C.GUARD, device=DEV),
           torch.full((SB,), C.GUARD, device=DEV), torch.full((SB,), -3, dtype=torch.int32, device=DEV))
    procs = P.PPOLogitsProcessors(V, DEV, repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[7], [3, 9]],
                                  forced_bos_token_id=4, forced_eos_token_id=eos, max_length=ST) if processing else None
    set_clock(clock, t)
    before = {k: w.clone() for k, w in wholes.items()}
    before_out = [o.clone() for o in out]
    P.ppo_sample_step(logits, temperature=0.7, top_k=20, top_p=0.9, min_length=3, ref_logits=ref, recorder=rec,
                      values=values, u=u, out=out, processors=procs, score_finished=True)
    torch.cuda.synchronize()
    for k, w in wholes.items():
        assert same(w, before[k]), k
    for o, b in zip(out, before_out):
        assert same(o, b)
    assert same(u_all, torch.full_like(u_all, C.GUARD))
    assert clock.record.tolist() == [t, T, 1, 0, 0, 0, 0, 0] and rec.t == 0


def test_a_shorter_record_buffer_bounds_the_live_steps():
    """a->T below the clock's T: t = a->T is dead although the clock would allow it."""
    V = 517
    logits = torch.zeros(SB, V, device=DEV)
    clock = P.T5DecodeClock(ST + 2, DEV)
    rec = P.PPORolloutRecorder(SB, ST + 2, DEV, pad_token_id=0, eos_token_id=1, clock=clock)
    rec.T = ST                                       # the entry is told the buffers hold ST columns
    set_clock(clock, ST)
    before = [rec.tokens.clone(), rec.logprobs.clone(), rec.unfinished.clone(), rec.lengths.clone()]
    ids, lp = P.ppo_sample_step(logits, ref_logits=logits, recorder=rec, u=torch.full((SB,), 0.5, device=DEV),
                                out=tuple(torch.full((SB,), 9, dtype=dt, device=DEV)
                                          for dt in (torch.int64, torch.float32, torch.float32, torch.int32)))
    assert ids.flatten().tolist() == [9] * SB and lp.tolist() == [9.0] * SB
    for now, was in zip([rec.tokens, rec.logprobs, rec.unfinished, rec.lengths], before):
        assert same(now, was)


# ------------------------------------------------------------------ 3. sampler, clock against host
PAD, EOS, BOS, TOK_A, TOK_B = 0, 1, 4, 11, 12
BAD_WORDS = [[7], [TOK_A, 9]]


def sampler_inputs(dtype, V, seed):
    """[T, B, V] policy and reference rows (made once per case): sigma 2 noise, with row 1 drawing
    eos at step 3 and row 2 walking A, B, A and then preferring B again — the bigram (A, B) that
    no_repeat_ngram_size = 2 bans at step 4."""
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(ST, SB, V, generator=g)
    x[:, :, EOS] = -30.0                                     # nobody else draws eos by chance
    x[3, 1, EOS] = 60.0
    for t, tok in ((1, TOK_A), (2, TOK_B), (3, TOK_A), (4, TOK_B)):
        x[t, 2, tok] = 60.0
    ref = x + 0.3 * torch.randn(ST, SB, V, generator=g)
    vals = torch.randn(ST, SB, generator=g)
    u = torch.rand(ST, SB, generator=g)
    prefix0 = torch.full((SB, 1), PAD, dtype=torch.int64)   # T5's decoder start token
    return x.to(dtype).to(DEV), ref.to(dtype).to(DEV), vals.to(DEV), u.to(DEV), prefix0.to(DEV)


def new_out():
    return (torch.full((SB,), -3, dtype=torch.int64, device=DEV), torch.full((SB,), C.GUARD, device=DEV),
            torch.full((SB,), C.GUARD, device=DEV), torch.full((SB,), -3, dtype=torch.int32, device=DEV))


def rollout_pair(dtype, V, processing, score_finished, table):
    x, ref, vals, u, prefix0 = sampler_inputs(dtype, V, 9000 + V)
    kw = dict(temperature=0.7, top_k=50, top_p=0.9, min_length=3, score_finished=score_finished)
    procs = None
    if processing:
        procs = P.PPOLogitsProcessors(V, DEV, repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=BAD_WORDS,
                                      forced_bos_token_id=BOS, forced_eos_token_id=EOS, max_length=7, eos_token_id=EOS)
        kw.update(processors=procs, prefix=prefix0)
    host = P.PPORolloutRecorder(SB, ST, DEV, pad_token_id=PAD, eos_token_id=EOS)
    clock = P.T5DecodeClock(ST, DEV, cur_len0=1)
    dev = P.PPORolloutRecorder(SB, ST, DEV, pad_token_id=PAD, eos_token_id=EOS, clock=clock)
    out_h, out_d = new_out(), new_out()
    for t in range(ST):
        P.ppo_sample_step(x[t], cur_len=1 + t, ref_logits=ref[t], recorder=host, values=vals[t], u=u[t], out=out_h,
                          **kw)
        P.ppo_sample_step(x[t], ref_logits=ref[t], recorder=dev, values=vals[t], u=u if table else u[t], out=out_d,
                          **kw)
        clock.advance()
        for a, b in zip(out_d, out_h):
            assert same(a, b), (t, "out")
        assert same(dev.unfinished, host.unfinished), t
        assert dev.t == 0
    for field in ("tokens", "logprobs", "ref_logprobs", "values", "lengths"):
        assert same(getattr(dev, field), getattr(host, field)), field
    assert clock.t == ST and clock.overrun == 0 and dev.sync_t() == ST == host.t
    return host


SAMPLER_CASES = [(dt, b, V) for dt in DTYPES for b, V in C.sampler_vocabs(dt)]


@pytest.mark.parametrize("score_finished", (False, True), ids=("ragged", "score_finished"))
@pytest.mark.parametrize("dtype,branch,V", SAMPLER_CASES, ids=lambda v: name(v) if isinstance(v, torch.dtype) else str(v))
def test_the_processing_step_with_the_clock_is_the_host_step(dtype, branch, V, score_finished):
    assert C.sampler_branch(V, dtype) == branch
    host = rollout_pair(dtype, V, True, score_finished, table=False)
    tok = host.tokens.cpu()
    assert tok[:, 0].tolist() == [BOS] * SB                      # forced bos at cur_len 1
    assert tok[1, 3] == EOS and int(host.lengths[1]) == 4        # a row draws eos mid-rollout
    assert tok[2, 1:4].tolist() == [TOK_A, TOK_B, TOK_A] and tok[2, 4] != TOK_B   # the repeated bigram is banned
    live_at_5 = (tok[:, 1:5] != EOS).all(dim=1)
    assert live_at_5.any() and (tok[live_at_5, 5] == EOS).all()  # forced eos at cur_len max_length - 1


@pytest.mark.parametrize("dtype,branch,V", SAMPLER_CASES, ids=lambda v: name(v) if isinstance(v, torch.dtype) else str(v))
def test_the_recording_step_with_the_clock_is_the_host_step(dtype, branch, V):
    host = rollout_pair(dtype, V, False, False, table=False)
    assert host.tokens[1, 3] == EOS and int(host.lengths[1]) == 4


@pytest.mark.parametrize("processing", (False, True), ids=("record", "proc"))
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_a_table_of_uniforms_is_the_host_step_fed_its_rows(dtype, processing):
    rollout_pair(dtype, 517, processing, True, table=True)


# ------------------------------------------------------------------ 4. C-ABI refusals with live tensors
def test_refusals_launch_nothing():
    d, inner, V = 64, ANH * 64, 517
    c = attn_case(torch.bfloat16, d)
    cache = attn_cache(c, torch.bfloat16, d, 0)
    out = torch.full((AB, inner), C.GUARD, dtype=torch.bfloat16, device=DEV)
    clock = P.T5DecodeClock(AMAX, DEV)
    q, kn, vn = (c["qkv"][:, i * inner:(i + 1) * inner] for i in range(3))
    ld = c["qkv"].stride(0)
    stream = _lib.stream_of(out)

    def attn(clock_ptr, **over):
        a = _lib.T5DecodeAttnArgs(
            q=q.data_ptr(), ldq=ld, k_new=kn.data_ptr(), ldk=ld, v_new=vn.data_ptr(), ldv=ld, k=cache.k.data_ptr(),
            v=cache.v.data_ptr(), bias_by_distance=c["table"].data_ptr(), key_mask=None, out=out.data_ptr(), B=AB,
            n_heads=ANH, d_kv=d, max_len=AMAX, t=0, dtype=_lib.BF16, mode=_lib.T5_ATTN_SELF)
        for k, v in over.items():
            setattr(a, k, v)
        return _lib.query("trlx_t5_decode_attn_dev", ctypes.byref(a), clock_ptr, stream)

    rec_ptr = clock.record.data_ptr()
    assert attn(None) == ERR_ARG and attn(rec_ptr + 4) == ERR_ARG
    assert attn(rec_ptr, mode=_lib.T5_ATTN_CROSS, k_new=None, v_new=None, bias_by_distance=None) == ERR_ARG
    # what the host-t entry refuses
    for over in (dict(d_kv=32), dict(dtype=_lib.I64), dict(q=None), dict(k_new=None), dict(ldq=inner - 8),
                 dict(out=out.data_ptr() + 2), dict(key_mask=rec_ptr), dict(max_len=0)):
        assert attn(rec_ptr, **over) == ERR_ARG, over
    assert _lib.query("trlx_t5_decode_attn_dev", None, rec_ptr, stream) == ERR_ARG
    torch.cuda.synchronize()
    assert same(out, torch.full_like(out, C.GUARD)) and same(cache.k, torch.full_like(cache.k, C.GUARD))
    assert attn(rec_ptr) == 0                                   # and the call they were built from runs
    torch.cuda.synchronize()
    assert not same(out, torch.full_like(out, C.GUARD))

    logits = torch.randn(SB, V, generator=torch.Generator().manual_seed(5)).to(DEV)
    sclock = P.T5DecodeClock(ST, DEV)
    rec = P.PPORolloutRecorder(SB, ST, DEV, pad_token_id=PAD, eos_token_id=EOS)
    for t_ in (rec.tokens, rec.logprobs, rec.ref_logprobs, rec.values, rec.lengths, rec.unfinished):
        t_.fill_(-9)
    rec.unfinished.fill_(1)
    u = torch.full((ST, SB), 0.5, device=DEV)
    o = new_out()

    def sample(dev=True, **over):
        a = _lib.PpoSampleProcArgs()
        a.logits, a.ld_logits, a.B, a.V, a.dtype = logits.data_ptr(), V, SB, V, _lib.F32
        a.temperature, a.top_p, a.min_tokens_to_keep, a.eos_token_id, a.pad_token_id = 1.0, 1.0, 1, EOS, PAD
        a.u, a.out_ids, a.out_logprobs, a.out_min_kept, a.out_kept_count = (u.data_ptr(), *(x.data_ptr() for x in o))
        a.unfinished = rec.unfinished.data_ptr()
        a.ref_logits, a.ld_ref, a.ref_dtype, a.T = logits.data_ptr(), V, _lib.F32, ST
        a.tokens, a.logprobs, a.ref_logprobs = rec.tokens.data_ptr(), rec.logprobs.data_ptr(), rec.ref_logprobs.data_ptr()
        a.ld_tokens = a.ld_logprobs = a.ld_ref_logprobs = a.ld_values = ST
        a.lengths = rec.lengths.data_ptr()
        a.repetition_penalty, a.forced_token_id = 1.0, -1
        da = _lib.PpoSampleDevArgs(clock=sclock.record.data_ptr(), forced_bos_token_id=-1, forced_eos_token_id=-1,
                                   max_length=0, u_ld=SB)
        for k, v in over.items():
            setattr(da if hasattr(da, k) else a, k, v)
        return _lib.query("trlx_ppo_sample_proc_dev", ctypes.byref(a), ctypes.byref(da) if dev else None, stream)

    arg_refusals = (dict(clock=None), dict(clock=sclock.record.data_ptr() + 4), dict(u_ld=SB - 1), dict(u_ld=-1),
                    dict(forced_bos_token_id=V), dict(forced_bos_token_id=-2), dict(forced_eos_token_id=V),
                    dict(forced_eos_token_id=-2), dict(forced_eos_token_id=EOS, max_length=0), dict(ref_logits=None),
                    dict(repetition_penalty=0.0), dict(no_repeat_ngram_size=-1), dict(temperature=0.0), dict(u=None),
                    dict(eos_token_id=V))
    assert sample(dev=False) == ERR_ARG
    for over in arg_refusals:
        assert sample(**over) == ERR_ARG, over
    for over in (dict(T=0), dict(ld_tokens=ST - 1), dict(prefix0=rec.tokens.data_ptr(), prefix0_len=3, prefix0_ld=2),
                 dict(prefix1=rec.tokens.data_ptr(), prefix1_ld=ST - 2), dict(ref_dtype=_lib.BF16), dict(V=0)):
        assert sample(**over) in (1, 3), over                   # TRLX_ERR_SHAPE / TRLX_ERR_DTYPE, as the host entry
    torch.cuda.synchronize()
    for t_ in (rec.tokens, rec.logprobs, rec.ref_logprobs, rec.values, rec.lengths):
        assert same(t_, torch.full_like(t_, -9))
    assert rec.unfinished.tolist() == [1] * SB and o[0].tolist() == [-3] * SB and o[3].tolist() == [-3] * SB
    # a->t, a->cur_len, a->forced_token_id and a->prefix1_len are not read: values the host entry refuses
    assert sample(t=ST + 5, cur_len=-4, forced_token_id=V + 3, prefix1_len=-2) == 0
    torch.cuda.synchronize()
    assert (rec.tokens[:, 0] >= 0).all() and (rec.tokens[:, 1:] == -9).all()


# ------------------------------------------------------------------ 5. one captured step replays a rollout
@pytest.mark.timeout(300)
def test_one_captured_step_replays_a_rollout():
    B, nH, d, T, S, D, V = 3, 2, 64, 6, 40, 128, 517
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(606)
    inner = nH * d
    w_qkv = (torch.randn(D, 3 * inner, generator=g) * D ** -0.5).to(dt).to(DEV)
    w_lm = (torch.randn(inner, V, generator=g) * 0.5).to(dt).to(DEV)
    w_ref = (w_lm.float().cpu() + 0.05 * torch.randn(inner, V, generator=g)).to(dt).to(DEV)
    xs = torch.randn(T, B, D, generator=g).to(dt).to(DEV)
    k_enc = (torch.randn(B, nH, S, d, generator=g) * d ** -0.25).to(dt).to(DEV)
    v_enc = torch.randn(B, nH, S, d, generator=g).to(dt).to(DEV)
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[0, 30:] = 0
    mask[1, :5] = 0
    mask[2, 17] = 0                                            # a hole
    mask = mask.to(DEV)
    table = P.t5_relative_bias_table(torch.randn(32, nH, generator=g).to(DEV), T)
    u = torch.rand(T, B, generator=g).to(DEV)
    prefix0 = torch.zeros(B, 1, dtype=torch.int64, device=DEV)
    procs = P.PPOLogitsProcessors(V, DEV, repetition_penalty=1.2, no_repeat_ngram_size=2, bad_words_ids=[[7], [3, 9]],
                                  forced_bos_token_id=4, forced_eos_token_id=1, max_length=T, eos_token_id=1)
    kw = dict(temperature=0.8, top_k=40, top_p=0.95, min_length=2, processors=procs, prefix=prefix0, score_finished=True)

    def step(x, cache, rec, t, clock=None):
        qkv = torch.matmul(x, w_qkv)
        q, kn, vn = (qkv[:, i * inner:(i + 1) * inner] for i in range(3))
        h = P.t5_decode_self_attention(q, kn, vn, cache, clock if clock is not None else t, table)
        h = P.t5_decode_cross_attention(h, k_enc, v_enc, mask)
        logits, ref = torch.matmul(h, w_lm), torch.matmul(h, w_ref)
        values = h[:, 0].contiguous()
        if clock is None:
            P.ppo_sample_step(logits, cur_len=1 + t, ref_logits=ref, recorder=rec, values=values, u=u[t], **kw)
        else:
            P.ppo_sample_step(logits, ref_logits=ref, recorder=rec, values=values, u=u, **kw)
            clock.advance()

    def state(cache, rec):
        return [t_.clone() for t_ in (cache.k, cache.v, rec.tokens, rec.logprobs, rec.ref_logprobs, rec.values,
                                      rec.lengths, rec.unfinished)]

    e_cache = P.T5DecodeKVCache(B, nH, d, T, dt, DEV)
    e_rec = P.PPORolloutRecorder(B, T, DEV, pad_token_id=0, eos_token_id=1)
    for t in range(T):
        step(xs[t], e_cache, e_rec, t)
    want = state(e_cache, e_rec)

    clock = P.T5DecodeClock(T, DEV)
    cache = P.T5DecodeKVCache(B, nH, d, T, dt, DEV)
    rec = P.PPORolloutRecorder(B, T, DEV, pad_token_id=0, eos_token_id=1, clock=clock)
    static_x = xs[0].clone()
    step(static_x, cache, rec, None, clock)                    # warm-up: every lazy initialisation is done
    torch.cuda.synchronize()
    rec.reset()
    cache.k.zero_()
    cache.v.zero_()
    assert clock.t == 0
    # Is capture available at all?  Decided on a torch op of a scratch tensor, before any of the
    # project's code runs under capture: only that may skip.
    scratch = torch.zeros(8, device=DEV)
    try:
        probe = torch.cuda.CUDAGraph()
        with torch.cuda.graph(probe):
            scratch.add_(1.0)
        probe.replay()
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.skip(f"graph capture is unavailable here: {e}")
    assert scratch.tolist() == [1.0] * 8
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # one stream, a linear chain of launches; a failure here fails the test
        step(static_x, cache, rec, None, clock)
    assert clock.t == 0                                        # a capture runs nothing
    after_T = None
    for i in range(T + 2):
        static_x.copy_(xs[min(i, T - 1)])
        graph.replay()
        if i == T - 1:
            torch.cuda.synchronize()
            after_T = state(cache, rec)
    torch.cuda.synchronize()
    got = state(cache, rec)
    for a, b in zip(got, want):
        assert same(a, b)
    for a, b in zip(got, after_T):                             # the two overrun replays changed nothing
        assert same(a, b)
    assert clock.t == T and clock.overrun == 2
    assert rec.t == 0 and rec.sync_t() == T and rec.t == T
