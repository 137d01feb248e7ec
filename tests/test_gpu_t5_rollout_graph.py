"""One captured decode step replayed per token as a real autoregressive rollout: t5_decode_embed
feeds the token drawn at the step before, both attentions skip the rows that have drawn eos
(live=recorder.unfinished), the recording step samples, clock.advance() ends the step.

Route (a) is eager with a host t and uses only what existed before: F.embedding of the recorder's
last column, t5_rmsnorm, the attentions without `live`, the recording step.  Route (c) is the new
step, run eagerly with the clock and as ONE captured graph replayed T + 2 times.  The record of a
rollout must be the same bits in all three: a finished row records pad, 0, 0 without reading its
logits (score_finished=False), so skipping its attention changes nothing that is recorded, and a
row of a matmul depends on that row of its input alone."""
import pytest
import torch
import torch.nn.functional as F

import trlx_t5_amd as P
import t5_rollout_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
L, NH, DKV, D, FF, V, S, T, B = 2, 2, 64, 128, 256, 97, 20, 12, 4
INNER = NH * DKV
DT = torch.bfloat16
PAD, EOS, START = 0, 1, 0
# Chosen against route (a) alone (which runs none of the new code) so that the precondition below
# holds: some row draws eos before column T - 2 and some row is still live at column T - 1.
SEED, EOS_SCALE = 0, 3.0
RECORD = ("tokens", "logprobs", "ref_logprobs", "values", "lengths", "unfinished")


class TinyDecoder:
    """L decoder layers on fixed weights; the projections are plain torch.matmul."""

    def __init__(self, seed, eos_scale):
        g = torch.Generator().manual_seed(seed)

        def w(*shape, scale):
            return (torch.randn(*shape, generator=g) * scale).to(DT).to(DEV)

        def ln():
            return (1.0 + 0.1 * torch.randn(D, generator=g)).to(DT).to(DEV)

        self.shared = w(V, D, scale=1.0)
        self.layers = [dict(qkv=w(D, 3 * INNER, scale=D ** -0.5), o=w(INNER, D, scale=INNER ** -0.5),
                            cq=w(D, INNER, scale=D ** -0.5), co=w(INNER, D, scale=INNER ** -0.5),
                            wi=w(D, 2 * FF, scale=D ** -0.5), wo=w(FF, D, scale=FF ** -0.5), ln=[ln(), ln(), ln()],
                            k_enc=w(B, NH, S, DKV, scale=DKV ** -0.25), v_enc=w(B, NH, S, DKV, scale=1.0))
                       for _ in range(L)]
        self.final_ln = ln()
        lm = torch.randn(D, V, generator=g) * D ** -0.5
        lm[:, EOS] *= eos_scale                                   # how often eos is drawn
        self.lm = lm.to(DT).to(DEV)
        self.ref_lm = (lm + 0.02 * torch.randn(D, V, generator=g)).to(DT).to(DEV)
        mask = torch.ones(B, S, dtype=torch.int64)
        mask[0, 15:] = 0
        mask[1, :3] = 0
        mask[2, 7] = 0                                            # a hole
        self.mask = mask.to(DEV)
        self.table = P.t5_relative_bias_table(torch.randn(32, NH, generator=g).to(DEV), T)
        self.u = torch.rand(T, B, generator=g).to(DEV)
        self.kw = dict(temperature=0.9, top_k=20, top_p=0.95)

    def state(self, clocked):
        clock = P.T5DecodeClock(T, DEV) if clocked else None
        caches = [P.T5DecodeKVCache(B, NH, DKV, T, DT, DEV) for _ in range(L)]
        rec = P.PPORolloutRecorder(B, T, DEV, pad_token_id=PAD, eos_token_id=EOS, clock=clock)
        return clock, caches, rec

    def body(self, h, y, caches, t, live):
        """The layers and the two lm_heads on the input row (h, its norm y) -> logits, ref, values."""
        kw = {} if live is None else dict(live=live)
        for i, w in enumerate(self.layers):
            qkv = torch.matmul(y, w["qkv"])
            q, kn, vn = (qkv[:, j * INNER:(j + 1) * INNER] for j in range(3))
            a = P.t5_decode_self_attention(q, kn, vn, caches[i], t, self.table, **kw)
            h, y = P.t5_add_rmsnorm(torch.matmul(a, w["o"]), h, w["ln"][1])
            c = P.t5_decode_cross_attention(torch.matmul(y, w["cq"]), w["k_enc"], w["v_enc"], self.mask, **kw)
            h, y = P.t5_add_rmsnorm(torch.matmul(c, w["co"]), h, w["ln"][2])
            f = P.t5_ff_act_packed(torch.matmul(y, w["wi"]))
            nxt = self.layers[i + 1]["ln"][0] if i + 1 < L else self.final_ln
            h, y = P.t5_add_rmsnorm(torch.matmul(f, w["wo"]), h, nxt)
        return torch.matmul(y, self.lm), torch.matmul(y, self.ref_lm), y[:, 0].contiguous()

    def step_a(self, state, t):
        """Eager, host t, built from the entries that existed before."""
        _, caches, rec = state
        tok = torch.full((B,), START, dtype=torch.int64, device=DEV) if t == 0 else rec.tokens[:, t - 1]
        h = F.embedding(tok, self.shared)
        y = P.t5_rmsnorm(h, self.layers[0]["ln"][0])
        logits, ref, values = self.body(h, y, caches, t, None)
        P.ppo_sample_step(logits, cur_len=1 + t, ref_logits=ref, recorder=rec, values=values, u=self.u[t], **self.kw)

    def step_c(self, state, out):
        """The new step: the same launches at every token."""
        clock, caches, rec = state
        h, y = P.t5_decode_embed(self.shared, rec, clock, START, self.layers[0]["ln"][0], out=out)
        logits, ref, values = self.body(h, y, caches, clock, rec.unfinished)
        P.ppo_sample_step(logits, ref_logits=ref, recorder=rec, values=values, u=self.u, **self.kw)
        clock.advance()


def route_a(dec):
    state = dec.state(False)
    for t in range(T):
        dec.step_a(state, t)
    torch.cuda.synchronize()
    return state


def precondition(rec):
    """Some row finishes before column T - 2 (its eos column is lengths - 1) and some row is still
    live at column T - 1: both the skip and the live path run until the last step."""
    lengths = rec.lengths.cpu()
    tokens = rec.tokens.cpu()
    early = [b for b in range(B) if lengths[b] - 1 < T - 2 and tokens[b, lengths[b] - 1] == EOS]
    late = [b for b in range(B) if not (tokens[b, :T - 1] == EOS).any()]
    return bool(early) and bool(late)


def snapshot(state):
    _, caches, rec = state
    return [getattr(rec, f).clone() for f in RECORD] + [x.clone() for c in caches for x in (c.k, c.v)]


def check_against_a(got, want):
    (_, caches, rec), (_, caches_a, rec_a) = got, want
    for f in RECORD:
        assert C.same(getattr(rec, f), getattr(rec_a, f)), f
    # the caches at every (row, column) that was live when written: the columns below the row's length
    lengths = rec_a.lengths.cpu().tolist()
    for i in range(L):
        for b in range(B):
            n = lengths[b]
            assert C.same(caches[i].k[b, :, :n], caches_a[i].k[b, :, :n]), (i, b, "k")
            assert C.same(caches[i].v[b, :, :n], caches_a[i].v[b, :, :n]), (i, b, "v")
            # a skipped row's later columns were never written
            assert not caches[i].k[b, :, n:].any() and not caches[i].v[b, :, n:].any(), (i, b, "skipped columns")


@pytest.fixture(scope="module")
def model_and_a():
    dec = TinyDecoder(SEED, EOS_SCALE)
    with torch.no_grad():
        want = route_a(dec)
    assert precondition(want[2]), (want[2].tokens.cpu(), want[2].lengths.cpu())
    assert want[2].t == T
    return dec, want


def test_the_new_step_run_eagerly_records_the_eager_rollout(model_and_a):
    """The clock route without a graph: a difference here is a kernel's, not the capture's."""
    dec, want = model_and_a
    state = dec.state(True)
    out = (torch.empty(B, D, dtype=DT, device=DEV), torch.empty(B, D, dtype=DT, device=DEV))
    with torch.no_grad():
        for _ in range(T):
            dec.step_c(state, out)
    torch.cuda.synchronize()
    check_against_a(state, want)
    assert state[0].t == T and state[0].overrun == 0


@pytest.mark.timeout(300)
def test_one_captured_step_replays_an_autoregressive_rollout(model_and_a):
    dec, want = model_and_a
    state = dec.state(True)
    clock, caches, rec = state
    out = (torch.empty(B, D, dtype=DT, device=DEV), torch.empty(B, D, dtype=DT, device=DEV))
    with torch.no_grad():
        dec.step_c(state, out)                                    # warm-up: every lazy initialisation is done
        torch.cuda.synchronize()
        rec.reset()
        for c in caches:
            c.k.zero_()
            c.v.zero_()
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
            dec.step_c(state, out)
        assert clock.t == 0                                       # a capture runs nothing
        after_T = None
        for i in range(T + 2):
            graph.replay()
            if i == T - 1:
                torch.cuda.synchronize()
                after_T = snapshot(state)
        torch.cuda.synchronize()
    check_against_a(state, want)
    for a, b in zip(snapshot(state), after_T):                    # the two overrun replays changed nothing
        assert C.same(a, b)
    assert clock.t == T and clock.overrun == 2
    assert rec.sync_t() == T
