"""The recording sampling step (csrc/ppo_sample.hip k_ppo_sample<.., true>, trlx_ppo_sample_record,
sampling.ppo_sample_step(ref_logits=, recorder=), rollout_store.PPORolloutRecorder) and
PPOHotPath.experience_from_logprobs.

  1  identity with the plain step: every reachable launch-table entry, both dtypes, four filters
  2  the reference log-prob against fp64 log_softmax: peaked rows, -inf entries, tokens 0 and
     V - 1, reference rows misaligned differently from the policy rows, head- / tail-only rows
  3  columns and bookkeeping over a 5-step loop: lengths, unfinished, finished rows (scored or
     not), values from fp32 / bf16, min_length
  4  experience_from_logprobs == experience, bit for bit, over lengths / mask / ctl / split-beta
  5  end to end: recorder bound to a hot path vs experience on the stacked logits; push_to
  6  refusals, each before any launch

Expected values are computed on the CPU in fp64 from the inputs as the kernel sees them."""
import pytest
import torch

import trlx_t5_amd as P
from ppo_record_checks import ATOL, RTOL, SHAPES, dname, plain, recorded, ref_want, same_snapshot, snapshot
from ppo_sample_checks import BF16, DEV, F32, LOGIT_POISON, esize, line_ld, place, row_split

pytestmark = pytest.mark.gpu
NEG = float("-inf")
FILTERS = [dict(top_k=1), dict(top_k=50), dict(top_p=0.9), dict(top_k=50, top_p=0.9)]


def rows(B, V, dtype, seed, scale=3.0, peak=False):
    """scale * randn; peak: +40 at one token per row, so the greedy token is unique (bf16 ties)."""
    g = torch.Generator().manual_seed(seed)
    x = scale * torch.randn(B, V, generator=g)
    if peak:
        x[torch.arange(B), torch.randint(0, V, (B,), generator=g)] = 40.0
    return x.to(dtype)


# ------------------------------------------------------------------ 1. identity with the plain step
@pytest.mark.parametrize("dtype,entry,V", SHAPES, ids=[f"{dname(d)}-N{e[0]}x{e[1]}-V{v}" for d, e, v in SHAPES])
def test_policy_outputs_identical_to_the_plain_step(dtype, entry, V):
    """Same logits, u and unfinished: ids, logprobs, min_kept_logit, kept_count and the updated
    unfinished are bit-identical to ppo_sample_step without a recorder, under every filter; the
    recorded column holds the same ids and logprobs."""
    B, T, eos, pad = 4, 2, 5, 0
    lg = rows(B, V, dtype, 11).to(DEV)
    ref = rows(B, V, dtype, 12).to(DEV)
    u = torch.tensor([0.03, 0.41, 0.77, 0.999], device=DEV)
    unf = torch.tensor([1, 1, 0, 1], dtype=torch.int64, device=DEV)
    for f in FILTERS:
        kw = dict(temperature=0.7, eos_token_id=eos, pad_token_id=pad, cur_len=3, min_length=0, **f)
        want = plain(lg, u, unf, **kw)
        rec = P.PPORolloutRecorder(B, T, DEV, pad, eos)
        rec.unfinished.copy_(unf)
        got = recorded(rec, lg, ref, u, **kw)
        for w, g in zip(want[:4], got):
            assert torch.equal(w, g), (f, w, g)
        assert torch.equal(want[4], rec.unfinished.cpu())
        assert rec.t == 1 and torch.equal(rec.tokens[:, 0].cpu(), want[0])
        assert torch.equal(rec.logprobs[:, 0].cpu(), want[1])
        live = unf.cpu() == 1
        torch.testing.assert_close(rec.ref_logprobs[:, 0].cpu().double()[live], ref_want(ref, want[0])[live],
                                   rtol=RTOL, atol=ATOL)
        assert float(rec.ref_logprobs[2, 0]) == 0.0 and int(rec.tokens[2, 0]) == pad


# ------------------------------------------------------------------ 2. the reference log-prob
def check_ref(lg, ref, want_ids=None):
    """Greedy step (top_k = 1: the token is the policy row's argmax) -> the recorded reference
    log-prob against fp64."""
    B, V = lg.shape
    rec = P.PPORolloutRecorder(B, 1, DEV, 0, None)
    u = torch.full((B,), 0.5, device=DEV)
    ids, lp, _, _ = recorded(rec, lg, ref, u, top_k=1)
    assert torch.equal(ids, lg.float().argmax(-1).cpu())
    if want_ids is not None:
        assert ids.tolist() == want_ids
    got = rec.ref_logprobs[:, 0].cpu().double()
    want = ref_want(ref, ids)
    print("ref_lp max abs err", float((got - want).abs().max()), "at |lp| up to", float(want.abs().max()))
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(lp.double(), ref_want(lg, ids), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("V", [37, 8065, 50257])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_ref_logprob_peaked_rows_inf_entries_and_edge_tokens(dtype, V):
    """Reference rows of sigma 4 with +8 at one token; a quarter of each row -inf, away from the
    drawn token; the drawn token at 0, at V - 1, and at the peaked reference token."""
    B = 6
    g = torch.Generator().manual_seed(V)
    lg = rows(B, V, dtype, 21).float()
    ref = 4.0 * torch.randn(B, V, generator=g)
    peak = torch.randint(0, V, (B,), generator=g)
    ref[torch.arange(B), peak] += 8.0
    tok = torch.randint(0, V, (B,), generator=g)
    tok[0], tok[1], tok[2] = 0, V - 1, peak[2]
    lg[torch.arange(B), tok] = 40.0           # the greedy token
    hole = torch.rand(B, V, generator=g) < 0.25
    hole[torch.arange(B), tok] = False
    hole[:3] = False                           # rows 0-2 stay free of -inf
    ref[hole] = NEG
    check_ref(lg.to(dtype).to(DEV), ref.to(dtype).to(DEV), want_ids=tok.tolist())


@pytest.mark.parametrize("V", [37, 8065, 50257])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_ref_rows_misaligned_differently_from_the_policy_rows(dtype, V):
    """Reference rows in a poisoned buffer (+1e30 around every row), one element past its start,
    with a row stride of 16k + one element (bf16: stride * 2 = 2 mod 16; fp32: 4 mod 16), so every
    row has another head / tail split and line shift; the policy rows are contiguous."""
    B, es = 5, esize(dtype)
    epv = 16 // es
    ld = (V + 2 * epv) // epv * epv + 1
    assert (ld * es) % 16 == es
    lg = rows(B, V, dtype, 31, peak=True).to(DEV)
    buf = torch.full((1 + B * ld + 64,), LOGIT_POISON, dtype=dtype, device=DEV)
    ref = buf.as_strided((B, V), (ld, 1), 1)
    ref.copy_(rows(B, V, dtype, 32, scale=4.0))
    phases = {(ref.data_ptr() + b * ld * es) % 16 for b in range(B)}
    assert len(phases) == min(B, 16 // es) and (lg.data_ptr() % 16, lg.stride(0)) != (ref.data_ptr() % 16, ref.stride(0))
    check_ref(lg, ref)


@pytest.mark.parametrize("kind", ["head", "tail", "both"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_ref_rows_of_a_head_only_a_tail_only_and_both(dtype, kind):
    """Rows that are only a head (3 elements before the first 16-B boundary), only a tail (3
    elements on a boundary), and head + 5 vectors + tail 2; poison around every row."""
    es = esize(dtype)
    epv = 16 // es
    phase, V = {"head": (16 - 3 * es, 3), "tail": (0, 3), "both": (16 - 3 * es, 3 + 5 * epv + 2)}[kind]
    head, nvec, tail0, tail, _ = row_split(phase, V, es)
    assert (head, nvec, tail) == {"head": (3, 0, 0), "tail": (0, 0, 3), "both": (3, 5, 2)}[kind]
    B = 3
    ref = place(rows(B, V, dtype, 41, scale=4.0), phase, line_ld(V, dtype), fill=LOGIT_POISON)
    lg = place(rows(B, V, dtype, 42, peak=True), 0, line_ld(V, dtype), fill=LOGIT_POISON)
    check_ref(lg, ref)


# ------------------------------------------------------------------ 3. columns and bookkeeping
@pytest.mark.parametrize("score_finished", [False, True], ids=["ragged", "scored"])
@pytest.mark.parametrize("V,dtype,vdtype", [(37, F32, F32), (8065, BF16, BF16), (8065, F32, BF16)],
                         ids=["V37-f32", "V8065-bf16-v16", "V8065-f32-v16"])
def test_columns_lengths_and_finished_rows_over_a_loop(V, dtype, vdtype, score_finished):
    """5 steps into T = 7 columns.  Rows 0 / 1 / 2 draw eos at steps 1 / 3 / 0 (its logit is +30
    there and -30 elsewhere, top_k = 5 keeps it out otherwise), rows 3-5 never do."""
    B, T, steps, eos, pad = 6, 7, 5, 7, 3
    eos_at = {0: 1, 1: 3, 2: 0}
    rec = P.PPORolloutRecorder(B, T, DEV, pad, eos)
    unf_plain = torch.ones(B, dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(5)
    kw = dict(top_k=5, temperature=0.9, eos_token_id=eos, pad_token_id=pad)
    first = snapshot(rec)
    assert bool((first[0]["tokens"] == pad).all()) and bool((first[0]["lengths"] == T).all())
    cols = []
    for t in range(steps):
        lg, ref = rows(B, V, dtype, 100 + t).float(), rows(B, V, dtype, 200 + t, scale=4.0).float()
        lg[:, eos] = -30.0
        for b, s in eos_at.items():
            if s == t:
                lg[b, eos] = 30.0
        lg, ref = lg.to(dtype).to(DEV), ref.to(dtype).to(DEV)
        vals = torch.randn(B, generator=g).to(vdtype).to(DEV)
        u = torch.rand(B, generator=g).to(DEV)
        was_live = unf_plain.cpu() == 1
        want = plain(lg, u, unf_plain, cur_len=t, **kw)
        unf_plain = want[4].to(DEV)
        got = recorded(rec, lg, ref, u, cur_len=t, values=vals, score_finished=score_finished, **kw)
        assert rec.t == t + 1
        assert torch.equal(got[0], want[0]) and torch.equal(rec.unfinished.cpu(), want[4])
        cols.append((was_live, want, lg, ref, vals))
    s, _ = snapshot(rec)
    for t, (live, want, lg, ref, vals) in enumerate(cols):
        ids = want[0]
        assert torch.equal(s["tokens"][:, t], ids) and bool((ids[~live] == pad).all())
        assert torch.equal(s["logprobs"][live, t], want[1][live])
        torch.testing.assert_close(s["ref_logprobs"][:, t].double()[live], ref_want(ref, ids)[live], rtol=RTOL,
                                   atol=ATOL)
        assert torch.equal(s["values"][live, t], vals.float().cpu()[live])
        if score_finished:   # log-softmax of both rows at pad, the value as given
            torch.testing.assert_close(s["logprobs"][:, t].double()[~live], ref_want(lg, ids)[~live], rtol=RTOL,
                                       atol=ATOL)
            torch.testing.assert_close(s["ref_logprobs"][:, t].double()[~live], ref_want(ref, ids)[~live],
                                       rtol=RTOL, atol=ATOL)
            assert torch.equal(s["values"][~live, t], vals.float().cpu()[~live])
        else:
            for k in ("logprobs", "ref_logprobs", "values"):
                assert bool((s[k][~live, t] == 0).all()), k
    for k in ("tokens", "logprobs", "ref_logprobs", "values"):   # columns not yet written
        assert torch.equal(s[k][:, steps:], first[0][k][:, steps:]), k
    is_eos = s["tokens"][:, :steps] == eos
    want_len = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((B,), T))
    assert want_len.tolist() == [2, 4, 1, T, T, T] and torch.equal(s["lengths"], want_len)
    assert s["unfinished"].tolist() == [0, 0, 0, 1, 1, 1]
    rec.reset()
    assert same_snapshot(snapshot(rec), first)


def test_min_length_suppression_with_a_recorder():
    """eos holds the largest logit in every row: while cur_len < min_length it is not drawn, at
    cur_len = min_length every row draws it and lengths becomes that column + 1."""
    B, T, V, eos, pad = 4, 5, 37, 9, 0
    rec = P.PPORolloutRecorder(B, T, DEV, pad, eos)
    for t in range(4):
        lg = rows(B, V, F32, 300 + t)
        lg[:, eos] = 30.0
        ids, _, _, _ = recorded(rec, lg.to(DEV), rows(B, V, F32, 400 + t).to(DEV), torch.full((B,), 0.5, device=DEV),
                                top_k=1, cur_len=t, min_length=3, eos_token_id=eos, pad_token_id=pad)
        if t < 3:
            lg[:, eos] = NEG
            assert torch.equal(ids, lg.argmax(-1)) and bool((rec.lengths == T).all())
        else:
            assert bool((ids == eos).all())
    assert rec.lengths.tolist() == [4] * B and rec.unfinished.tolist() == [0] * B


# ------------------------------------------------------------------ 4. experience_from_logprobs
def hot_inputs(B, T, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: torch.randn(B, T, V, generator=g).to(dtype).to(DEV)  # noqa: E731
    d = dict(logits=mk(), ref_logits=mk(), new_logits=mk(), labels=torch.randint(0, V, (B, T), generator=g).to(DEV),
             old_values=torch.randn(B, T, generator=g).to(DEV), scores=(torch.rand(B, generator=g) * 8 - 4).to(DEV))
    d["values"] = d["old_values"] + 0.1
    return d


def make_hp(B, T, V, dtype, ctl, split):
    c = P.PPOControlState(DEV, scale_reward="running", cliprange_reward=10) if ctl else None
    return P.PPOHotPath(P.PPOConfig(), B, T, V, dtype, DEV, kl_coef=0.05, ctl=c, split_beta=split)


def hp_state(hp, loss_out):
    torch.cuda.synchronize()
    return [hp.rewards.clone(), hp.adv_raw.clone(), hp.returns.clone(), hp.adv_stats.clone()] + \
        [t.clone() for t in loss_out]


@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split"])
@pytest.mark.parametrize("ctl", [False, True], ids=["noctl", "ctl"])
@pytest.mark.parametrize("ragged", ["full", "lengths", "mask"])
@pytest.mark.parametrize("B,T,V,dtype", [(4, 6, 37, F32), (4, 2, 50257, BF16)], ids=["V37", "V50257"])
def test_experience_from_logprobs_equals_experience(B, T, V, dtype, ragged, ctl, split):
    """experience() on [B, T, V] logits, its lp_old / ref_lp cloned into experience_from_logprobs
    on an identically built hot path: rewards, raw advantages, returns, the whitening record and
    a following policy_loss (loss, stats, dlogits, dvalues) are bit-identical."""
    d = hot_inputs(B, T, V, dtype, 7)
    lengths = torch.tensor([T, 1, max(T - 2, 1), T][:B], device=DEV) if ragged == "lengths" else None
    mask = None
    if ragged == "mask":
        mask = torch.ones(B, T, dtype=torch.int64, device=DEV)
        mask[1, T - 1:] = 0
        mask[2, 1:] = 0
    a, b = make_hp(B, T, V, dtype, ctl, split), make_hp(B, T, V, dtype, ctl, split)
    lp, rlp = a.experience(d["logits"], d["ref_logits"], d["labels"], d["old_values"], d["scores"], lengths=lengths,
                           mask=mask)
    lp, rlp = lp.clone(), rlp.clone()
    sa = hp_state(a, a.policy_loss(d["new_logits"], d["labels"], d["values"], d["old_values"], mask=mask))
    b.lp_old.fill_(7.0)
    out = b.experience_from_logprobs(d["labels"], d["old_values"], d["scores"], logprobs=lp, ref_logprobs=rlp,
                                     lengths=lengths, mask=mask)
    assert out[0] is b.lp_old and out[1] is b.ref_lp and torch.equal(b.lp_old, lp) and torch.equal(b.ref_lp, rlp)
    sb = hp_state(b, b.policy_loss(d["new_logits"], d["labels"], d["values"], d["old_values"], mask=mask))
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert torch.equal(x, y), i


# ------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("V,dtype", [(37, F32), (8065, BF16)], ids=["V37-f32", "V8065-bf16"])
def test_recorder_route_against_experience_on_the_stacked_logits(V, dtype):
    """A recorder bound to a hot path, T recording steps on seeded slabs, experience_from_logprobs;
    against experience() on the stacked [B, T, V] slabs with labels = the recorded tokens.  The
    two row kernels sum in different orders: rtol 1e-5 / atol 1e-6.  Then push_to + collate."""
    B, T, pad, eos = 4, 5, 0, 2
    hp = P.PPOHotPath(P.PPOConfig(), B, T, V, dtype, DEV, kl_coef=0.05)
    rec = P.PPORolloutRecorder(B, T, DEV, pad, eos, hot_path=hp)
    assert rec.logprobs is hp.lp_old and rec.ref_logprobs is hp.ref_lp
    g = torch.Generator().manual_seed(9)
    slabs, refs = torch.empty(B, T, V, dtype=dtype, device=DEV), torch.empty(B, T, V, dtype=dtype, device=DEV)
    for t in range(T):
        slabs[:, t] = rows(B, V, dtype, 500 + t).to(DEV)
        refs[:, t] = rows(B, V, dtype, 600 + t).to(DEV)
        refs[:, t, eos] = -30.0
        slabs[:, t, eos] = -30.0
        if t == 2:
            slabs[1, t, eos] = 30.0   # row 1 draws eos at step 2
        P.ppo_sample_step(slabs[:, t], ref_logits=refs[:, t], recorder=rec, values=torch.randn(B, generator=g).to(DEV),
                          u=torch.rand(B, generator=g).to(DEV), top_k=20, cur_len=t)
    assert rec.t == T and rec.lengths.tolist() == [T, 3, T, T]
    scores = (torch.rand(B, generator=g) * 8 - 4).to(DEV)
    old_values = rec.values.clone()
    hp.experience_from_logprobs(rec.tokens, old_values, scores, lengths=rec.lengths)
    torch.cuda.synchronize()
    got = [hp.rewards.cpu(), hp.adv_raw.cpu(), hp.returns.cpu()]
    ref_hp = P.PPOHotPath(P.PPOConfig(), B, T, V, dtype, DEV, kl_coef=0.05)
    ref_hp.experience(slabs, refs, rec.tokens, old_values, scores, lengths=rec.lengths)
    torch.cuda.synchronize()
    for x, y in zip(got, [ref_hp.rewards.cpu(), ref_hp.adv_raw.cpu(), ref_hp.returns.cpu()]):
        torch.testing.assert_close(x, y, rtol=RTOL, atol=ATOL)
    store = P.PPORolloutStorage(pad, DEV)
    query = torch.randint(3, V, (B, 4), generator=g).to(DEV)
    rec.push_to(store, query, hp.rewards)
    batch = store.collate(torch.arange(B, device=DEV), torch.arange(B).numpy())
    torch.cuda.synchronize()
    assert len(store) == B and torch.equal(batch.query_tensors, query)
    assert torch.equal(batch.response_tensors, rec.tokens) and torch.equal(batch.logprobs, rec.logprobs)
    assert torch.equal(batch.values, rec.values) and torch.equal(batch.rewards, hp.rewards)


# ------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_any_launch():
    B, T, V, pad, eos = 4, 2, 37, 0, 1
    lg, ref = rows(B, V, F32, 1).to(DEV), rows(B, V, F32, 2).to(DEV)
    rec = P.PPORolloutRecorder(B, T, DEV, pad, eos)
    rec.tokens.fill_(11)   # any launch would overwrite a column
    before = snapshot(rec)
    bad = [dict(ref_logits=ref), dict(recorder=rec),                                  # one without the other
           dict(ref_logits=ref.to(BF16), recorder=rec),                               # dtype mismatch
           dict(ref_logits=ref[:, :V - 1], recorder=rec), dict(ref_logits=ref[:B - 1], recorder=rec),
           dict(ref_logits=ref, recorder=P.PPORolloutRecorder(B + 1, T, DEV, pad, eos)),  # another B
           dict(ref_logits=ref, recorder=rec, values=torch.zeros(B + 1, device=DEV)),
           dict(ref_logits=ref, recorder=rec, pad_token_id=pad + 1),
           dict(ref_logits=ref, recorder=rec, temperature=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            P.ppo_sample_step(lg, **kw)
    with pytest.raises(ValueError):   # the entry's own check: the two rows' dtype codes differ
        P._lib.call("trlx_ppo_sample_record", lg.data_ptr(), V, P._lib.F32, B, V, 1.0, 0, 1.0, 1, 0, 0, eos, pad,
                    torch.rand(B, device=DEV).data_ptr(), rec.tokens.data_ptr(), rec.logprobs.data_ptr(),
                    rec.logprobs.data_ptr(), rec.lengths.data_ptr(), None, ref.data_ptr(), V, P._lib.BF16, 0, T,
                    rec.tokens.data_ptr(), T, rec.logprobs.data_ptr(), T, rec.ref_logprobs.data_ptr(), T, None, T,
                    None, 0, None, 0, P._lib.stream_of(lg))
    for t_bad, ld_bad in ((T, T), (-1, T), (0, T - 1)):   # t outside [0, T), a stride below T
        with pytest.raises(ValueError):
            P._lib.call("trlx_ppo_sample_record", lg.data_ptr(), V, P._lib.F32, B, V, 1.0, 0, 1.0, 1, 0, 0, eos, pad,
                        torch.rand(B, device=DEV).data_ptr(), rec.tokens.data_ptr(), rec.logprobs.data_ptr(),
                        rec.logprobs.data_ptr(), rec.lengths.data_ptr(), None, ref.data_ptr(), V, P._lib.F32, t_bad,
                        T, rec.tokens.data_ptr(), ld_bad, rec.logprobs.data_ptr(), T, rec.ref_logprobs.data_ptr(), T,
                        None, T, None, 0, None, 0, P._lib.stream_of(lg))
    torch.cuda.synchronize()
    assert same_snapshot(snapshot(rec), before)
    for _ in range(T):   # fill it: the full recorder refuses
        P.ppo_sample_step(lg, ref_logits=ref, recorder=rec)
    full = snapshot(rec)
    with pytest.raises(ValueError, match="full"):
        P.ppo_sample_step(lg, ref_logits=ref, recorder=rec)
    torch.cuda.synchronize()
    assert same_snapshot(snapshot(rec), full) and rec.t == T


def test_experience_from_logprobs_refuses_a_pending_pipeline_batch_and_bad_logprobs():
    B, T, V = 4, 3, 37
    d = hot_inputs(B, T, V, F32, 3)
    hp = make_hp(B, T, V, F32, False, False)
    with pytest.raises(ValueError):
        hp.experience_from_logprobs(d["labels"], d["old_values"], d["scores"], logprobs=torch.zeros(B, T + 1, device=DEV))
    with pytest.raises(ValueError):
        hp.experience_from_logprobs(d["labels"], d["old_values"], d["scores"],
                                    ref_logprobs=torch.zeros(B, T, dtype=torch.bfloat16, device=DEV))
    assert hp.pipeline_step(d["logits"], d["ref_logits"], d["new_logits"], d["labels"], d["old_values"], d["values"],
                            d["scores"]) is None
    torch.cuda.synchronize()
    lp, pending = hp.lp_old.clone(), hp._pending
    with pytest.raises(RuntimeError, match="pending batch"):
        hp.experience_from_logprobs(d["labels"], d["old_values"], d["scores"], logprobs=torch.zeros(B, T, device=DEV))
    torch.cuda.synchronize()
    assert hp._pending is pending and torch.equal(hp.lp_old, lp)
    assert hp.pipeline_flush() is not None
