"""trlx_t5_decode_linear_rows on the GPU (csrc/t5_decode_linear_rows.hip; t5_decode_linear(live=,
split_rows=)): the decode-step projection with the rows spread over workgroups and the finished rows
skipped, against the entry it restates (trlx_t5_decode_linear).

The main comparison is equality of the raw bits: a row's output does not depend on the tile, pass or
workgroup it lands in, so every live row must carry the bits of the default call, at every shape and
form.  `out` sits inside guard margins that are checked afterwards, and every operand is the test's own
memory: the NaN test below is a value test on valid rows, not an out-of-bounds probe."""
import ctypes
import sys

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_rollout_checks as C
import t5_decode_linear_checks as L

TDL = sys.modules["trlx_t5_amd.t5_decode_linear"]
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
PAD = 8                                         # row stride = columns + PAD: strided rows on the 16-byte grid
RB = TDL.ROWS_PER_BLOCK
MS = (1, 15, 16, 17, RB - 1, RB, RB + 1, 2 * RB + 1, 257)
NS = (16, 48)
KS = (96, 1056)                                 # both forms of the norm's sum; 1056: wave 0 takes a third turn
LIVE_SHAPES = ((48, 96), (16, 1056))            # (N, K) of the live-pattern cases
_INPUTS = {}


def strided(t):
    """A copy of t [rows, cols] as a row-strided view inside guard margins: (whole, view)."""
    rows, cols = t.shape
    whole, view = C.with_margins((rows, cols), t.dtype, DEV, cols + PAD, ld=cols + PAD)
    view.copy_(t)
    return whole, view


def guarded_out(M, N):
    return C.with_margins((M, N), BF, DEV, N + PAD, ld=N + PAD)


def margins_kept(whole, view):
    """Everything of `whole` outside `view`'s elements still holds the guard."""
    probe = whole.clone()
    lo = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    rows, cols = view.shape
    probe[lo:lo + rows * view.stride(0)].view(rows, view.stride(0))[:, :cols] = C.GUARD
    return C.same(probe, torch.full_like(probe, C.GUARD))


def inputs(M, N, K, gated):
    """x, w, nw, res of one shape on the device, made once and never modified."""
    key = (M, N, K, gated)
    if key not in _INPUTS:
        _INPUTS[key] = L.inputs(M, N, K, gated, seed=1000 * K + 10 * N + M, device=DEV)
    return _INPUTS[key]


def keywords(combo, nw, res):
    norm, (_, with_res, act, gated) = combo
    return dict(norm_weight=nw if norm else None, residual=res if with_res else None, act=act, gated=gated)


def patterns(M):
    """name -> live [M] int64 on the device; nonzero = live."""
    idx = torch.arange(M)
    g = torch.Generator().manual_seed(4000 + M)
    p = {"all": torch.ones(M), "none": torch.zeros(M), "row_0": idx == 0, "last_row": idx == M - 1,
         "every_other": idx % 2 == 0, "first_rb_plus_1_dead": idx > RB, "bernoulli": torch.rand(M, generator=g) < 0.5}
    return {k: (v.to(torch.int64) * 5).to(DEV) for k, v in p.items()}


def dead_rows_want(res, on, with_res, like):
    return res[~on] if with_res else torch.zeros_like(like[~on])


def test_the_constants_are_the_librarys():
    g = TDL.rows_geometry()
    assert g["rows_per_block"] == RB and g["max_m_live"] == TDL.MAX_M_LIVE
    assert sorted(set(MS)) == sorted({1, 15, 16, 17, RB - 1, RB, RB + 1, 2 * RB + 1, 257})
    assert KS[0] <= TDL.geometry()["norm_wave_row_max_k"] < KS[1]


# ------------------------------------------------------------------ bit-equality without live
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_split_rows_equals_the_existing_entry_bit_for_bit(combo):
    gated = combo[1][3]
    for M in MS:
        for N in NS:
            for K in KS:
                x, w, nw, res = inputs(M, N, K, gated)
                kw = keywords(combo, nw, res)
                o_all, want = guarded_out(M, N)
                P.t5_decode_linear(x, w, out=want, **kw)
                a_all, got = guarded_out(M, N)
                assert P.t5_decode_linear(x, w, out=got, split_rows=True, **kw) is got
                b_all, again = guarded_out(M, N)
                P.t5_decode_linear(x, w, out=again, split_rows=True, **kw)
                assert C.same(got.contiguous(), want.contiguous()), (M, N, K)
                assert C.same(again.contiguous(), got.contiguous()), (M, N, K, "two calls differ")
                assert margins_kept(a_all, got) and margins_kept(b_all, again) and margins_kept(o_all, want), (M, N, K)


@pytest.mark.parametrize("norm", (False, True), ids=("plain", "norm"))
def test_a_last_position_view_and_an_in_place_residual(norm):
    for M in MS:
        N, K = 48, 96
        x, w, nw, res = inputs(M, N, K, False)
        hseq = torch.randn(M, 3, K, generator=torch.Generator().manual_seed(M)).to(BF).to(DEV)
        hseq[:, -1, :] = x
        view = hseq[:, -1, :]                                     # rows 3 K apart, read in place
        nkw = dict(norm_weight=nw if norm else None)
        want = P.t5_decode_linear(x, w, **nkw)
        assert C.same(P.t5_decode_linear(view, w, split_rows=True, **nkw), want), M
        r_all, r_old = strided(res)
        P.t5_decode_linear(x, w, residual=r_old, out=r_old, **nkw)
        s_all, r_new = strided(res)
        assert P.t5_decode_linear(view, w, residual=r_new, out=r_new, split_rows=True, **nkw) is r_new
        assert C.same(r_new.contiguous(), r_old.contiguous()), M
        assert margins_kept(s_all, r_new) and margins_kept(r_all, r_old), M


# ------------------------------------------------------------------ live patterns
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_live_rows_keep_their_bits_and_dead_rows_follow_the_rule(combo):
    _, (_, with_res, _, gated) = combo
    for M in MS:
        for N, K in LIVE_SHAPES:
            x, w, nw, res = inputs(M, N, K, gated)
            kw = keywords(combo, nw, res)
            want = P.t5_decode_linear(x, w, **kw)
            for name, live in patterns(M).items():
                on = live != 0
                what = (M, N, K, name)
                o_all, out = guarded_out(M, N)
                assert P.t5_decode_linear(x, w, out=out, live=live, **kw) is out
                assert C.same(out[on], want[on]), what + ("live rows",)
                assert C.same(out[~on], dead_rows_want(res, on, with_res, want)), what + ("dead rows",)
                assert margins_kept(o_all, out), what
                if with_res:                                      # in place: a dead row is left untouched
                    r_all, r = strided(res)
                    before = r_all.clone()
                    assert P.t5_decode_linear(x, w, **dict(kw, residual=r), out=r, live=live) is r
                    assert C.same(r[on], want[on]), what + ("in place, live rows",)
                    assert C.same(r[~on], res[~on]), what + ("in place, dead rows",)
                    untouched = before.clone()
                    lo = (r.data_ptr() - r_all.data_ptr()) // 2
                    mine = untouched[lo:lo + M * r.stride(0)].view(M, r.stride(0))
                    mine[on, :N] = want[on]
                    assert C.same(r_all, untouched), what + ("in place: anything but the live rows was written",)
                assert (live != 0).equal(on) and int(live.max()) in (0, 5), what


# ------------------------------------------------------------------ nothing of a dead row is read
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_a_dead_rows_x_reaches_no_output(combo):
    _, (_, with_res, _, gated) = combo
    nan, inf = float("nan"), float("inf")
    for M in (17, RB + 1, 257):
        for N, K in LIVE_SHAPES:
            x, w, nw, res = inputs(M, N, K, gated)
            kw = keywords(combo, nw, res)
            want = P.t5_decode_linear(x, w, **kw)
            for name in ("every_other", "first_rb_plus_1_dead", "bernoulli", "last_row"):
                live = patterns(M)[name]
                on = live != 0
                bad = x.clone()
                fill = torch.tensor([nan, inf, -inf, nan], dtype=BF, device=DEV).repeat(K // 4)
                bad[~on] = fill
                bad[~on, ::7] = -nan
                got = P.t5_decode_linear(bad, w, live=live, **kw)
                assert C.same(got[on], want[on]), (M, N, K, name, "live rows")
                assert torch.isfinite(got.float()).all(), (M, N, K, name, "a dead row's x reached an output")
                assert C.same(got[~on], dead_rows_want(res, on, with_res, want)), (M, N, K, name, "dead rows")


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_accuracy_of_the_live_rows_against_the_float64_oracle(combo):
    norm, (_, with_res, act, gated) = combo
    M, N, K = 65, 48, 256
    x, w, nw, res = inputs(M, N, K, gated)
    live = patterns(M)["bernoulli"]
    on = live != 0
    okw = dict(norm_w=nw if norm else None, residual=res if with_res else None, act=act, gated=gated)
    ref = L.oracle(x, w, **okw)[on]
    e_unfused = L.max_err(L.unfused(x, w, **okw)[on], ref)
    got = P.t5_decode_linear(x, w, live=live, split_rows=True, **keywords(combo, nw, res))
    e_kernel = L.max_err(got[on], ref)
    limit = L.bound(e_unfused, ref)
    print(f"{L.combo_name(combo)}: e_kernel {e_kernel:.4g} e_unfused {e_unfused:.4g} bound {limit:.4g} "
          f"ratio {e_kernel / limit:.3f}")
    assert int(on.sum()) >= 16 and torch.isfinite(got.float()).all()
    assert e_kernel <= limit, (e_kernel, e_unfused, limit)


# ------------------------------------------------------------------ refusals
def _args(xt, wt, ot, nw=None, res=None, live=None, act=_lib.T5_ACT_NONE, gated=0, dtype=_lib.BF16, **over):
    """The arguments of a valid call on these tensors (live: a tensor or an address), then `over` on top."""
    M, K = xt.shape
    N = ot.shape[1]
    live = _lib.ptr(live) if live is None or isinstance(live, torch.Tensor) else live
    kw = dict(x=xt.data_ptr(), ld_x=xt.stride(0), weight=wt.data_ptr(), ld_w=wt.stride(0), norm_weight=_lib.ptr(nw),
              residual=_lib.ptr(res), ld_residual=N if res is None else res.stride(0), out=ot.data_ptr(),
              ld_out=ot.stride(0), M=M, K=K, N=N, eps=1e-6, dtype=dtype, act=act, gated=gated, live=live, reserved=0)
    kw.update(over)
    return _lib.T5DecodeLinearRowsArgs(**kw)


def test_every_refusal_returns_its_status_and_leaves_out_untouched():
    lib = _lib.load()
    M, N, K = 3, 16, 64
    x, w, nw, res = L.inputs(M, N, K, True, seed=9, device=DEV)
    (_, xs), (_, ws), (_, rs) = strided(x), strided(w), strided(res)
    o_all, out = guarded_out(M, N)
    live = torch.ones(M + 1, dtype=torch.int64, device=DEV)
    words = torch.ones(64, dtype=torch.int64, device=DEV)         # 512 bytes: room for a [3, 24] bf16 out on top of live
    big = torch.zeros(M, L.NORM_MAX_K + 32, dtype=BF, device=DEV)
    wbig = torch.zeros(N, L.NORM_MAX_K + 32, dtype=BF, device=DEV)
    nwbig = torch.ones(L.NORM_MAX_K + 32, dtype=BF, device=DEV)
    stream = _lib.stream_of(out)
    w1 = ws[:N]
    cases = [
        # the new ones
        ("live off 8 bytes", _args(xs, w1, out, live=live.data_ptr() + 4), C.ERR_ARG),
        ("live overlaps out", _args(xs, w1, out, live=words, out=words.data_ptr() + 16, ld_out=N + PAD), C.ERR_ARG),
        ("live inside out", _args(xs, w1, out, live=words.data_ptr() + 32, out=words.data_ptr(), ld_out=N + PAD), C.ERR_ARG),
        ("M above the live limit", _args(xs, w1, out, live=live, M=TDL.MAX_M_LIVE + 1), C.ERR_SHAPE),
        ("M above the grid", _args(xs, w1, out, M=65535 * RB + 1), C.ERR_SHAPE),
        # what trlx_t5_decode_linear refuses, with its statuses
        ("NULL args", None, C.ERR_ARG),
        ("NULL x", _args(xs, w1, out, x=None), C.ERR_ARG),
        ("NULL weight", _args(xs, w1, out, weight=None), C.ERR_ARG),
        ("NULL out", _args(xs, w1, out, live=live, out=None), C.ERR_ARG),
        ("fp32", _args(xs, w1, out, dtype=_lib.F32), C.ERR_DTYPE),
        ("M 0", _args(xs, w1, out, live=live, M=0), C.ERR_SHAPE),
        ("K not a multiple of 32", _args(xs, w1, out, K=48), C.ERR_SHAPE),
        ("K 0", _args(xs, w1, out, K=0), C.ERR_SHAPE),
        ("K above 16384", _args(xs, w1, out, K=16416, ld_x=16424, ld_w=16424), C.ERR_SHAPE),
        ("N not a multiple of 16", _args(xs, w1, out, N=8), C.ERR_SHAPE),
        ("K above 8192 with a norm weight", _args(big, wbig, out, nw=nwbig), C.ERR_SHAPE),
        ("x off 16 bytes", _args(xs, w1, out, x=xs.data_ptr() + 2), C.ERR_ARG),
        ("weight off 16 bytes", _args(xs, w1, out, weight=w1.data_ptr() + 8), C.ERR_ARG),
        ("out off 16 bytes", _args(xs, w1, out, live=live, out=out.data_ptr() + 4), C.ERR_ARG),
        ("norm weight off 16 bytes", _args(xs, w1, out, norm_weight=nw.data_ptr() + 2), C.ERR_ARG),
        ("residual off 16 bytes", _args(xs, w1, out, res=rs, residual=rs.data_ptr() + 2), C.ERR_ARG),
        ("x stride below K", _args(xs, w1, out, ld_x=K - 8), C.ERR_STRIDE),
        ("x stride off the grid", _args(xs, w1, out, ld_x=K + 4), C.ERR_STRIDE),
        ("weight stride off the grid", _args(xs, w1, out, ld_w=K + 2), C.ERR_STRIDE),
        ("out stride below N", _args(xs, w1, out, ld_out=8), C.ERR_STRIDE),
        ("out stride off the grid", _args(xs, w1, out, live=live, ld_out=N + 4), C.ERR_STRIDE),
        ("residual stride off the grid", _args(xs, w1, out, res=rs, ld_residual=N + 4), C.ERR_STRIDE),
        ("out overlaps x", _args(xs, w1, out, out=xs.data_ptr(), ld_out=xs.stride(0)), C.ERR_ARG),
        ("out overlaps weight", _args(xs, w1, out, live=live, out=w1.data_ptr(), ld_out=w1.stride(0)), C.ERR_ARG),
        ("out overlaps the norm weight", _args(xs, w1, out, nw=nw, out=nw.data_ptr(), M=1, N=16), C.ERR_ARG),
        ("out overlaps residual, shifted", _args(xs, w1, out, res=rs, out=rs.data_ptr() + 16, ld_out=rs.stride(0)), C.ERR_ARG),
        ("out is residual with another stride", _args(xs, w1, out, res=rs, live=live, out=rs.data_ptr(),
                                                     ld_out=rs.stride(0) + 8), C.ERR_ARG),
        ("both epilogues", _args(xs, w1, out, res=rs, act=_lib.T5_ACT_SILU), C.ERR_ARG),
        ("gated without an act", _args(xs, ws, out, gated=1), C.ERR_ARG),
        ("an unknown act", _args(xs, w1, out, act=7), C.ERR_ARG),
        ("eps NaN", _args(xs, w1, out, nw=nw, eps=float("nan")), C.ERR_ARG),
    ]
    snapshot = [t.clone() for t in (xs, ws, rs, nw, words, live)]
    for name, a, status in cases:
        rc = lib.trlx_t5_decode_linear_rows(None if a is None else ctypes.byref(a), stream)
        assert rc == status, (name, rc, lib.trlx_last_error())
        assert lib.trlx_last_error(), name
    torch.cuda.synchronize()
    assert C.same(o_all, torch.full_like(o_all, C.GUARD))
    assert all(C.same(a, b) for a, b in zip((xs, ws, rs, nw, words, live), snapshot))
    # the same blocks without the fault are taken: with live, without it, live right behind out
    for a in (_args(xs, w1, out, live=live), _args(xs, w1, out), _args(xs, w1, out, live=live.data_ptr() + 8)):
        assert lib.trlx_t5_decode_linear_rows(ctypes.byref(a), stream) == 0, lib.trlx_last_error()
    torch.cuda.synchronize()
    assert C.same(out.contiguous(), P.t5_decode_linear(xs, w1)) and margins_kept(o_all, out)
    # the python entry refuses a bad live before the library is asked
    for bad in (live, live[:M].to(torch.int32), live[:M].cpu(), torch.ones(2 * M, dtype=torch.int64, device=DEV)[::2]):
        with pytest.raises(ValueError, match="live"):
            P.t5_decode_linear(xs, w1, live=bad)


def test_the_defaults_take_the_entry_they_always_took(monkeypatch):
    x, w, nw, res = inputs(17, 48, 96, False)
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    live = torch.ones(17, dtype=torch.int64, device=DEV)
    P.t5_decode_linear(x, w)
    P.t5_decode_linear(x, w, live=None, split_rows=False)
    P.t5_decode_linear(x, w, split_rows=True)
    P.t5_decode_linear(x, w, live=live)
    assert called == ["trlx_t5_decode_linear"] * 2 + ["trlx_t5_decode_linear_rows"] * 2


# ------------------------------------------------------------------ the captured rollout
NL_, B_, D_, NH_, DKV_, F_, S_, T_, V_ = 2, 5, 64, 2, 64, 96, 7, 6, 23
INNER_ = NH_ * DKV_
PAD_ID, EOS_ID, START_ID = 0, 1, 0
# Chosen against the eager route alone (which runs none of the new code) so that the precondition of
# the test holds: at least two rows draw eos before column T - 1 and at least two never do.
SEED_, EOS_SCALE_ = 2, 3.0
RECORD = ("tokens", "logprobs", "ref_logprobs", "values", "lengths", "unfinished")


class TinyFusedDecoder:
    """NL_ decoder layers (gated gelu_new) on the 8-launch layer, the lm_heads and the sampler."""

    def __init__(self, seed, eos_scale):
        g = torch.Generator().manual_seed(seed)

        def rnd(*shape, scale=1.0):
            return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)

        self.blocks = [P.T5DecodeBlockWeights.from_state_dict(
            L.hf_block_state_dict(D_, INNER_, F_, True, seed=100 * seed + i, device=DEV), "decoder.block.0.") for i in range(NL_)]
        self.shared = rnd(V_, D_)
        self.k_enc = [rnd(B_, NH_, S_, DKV_, scale=DKV_ ** -0.25) for _ in range(NL_)]
        self.v_enc = [rnd(B_, NH_, S_, DKV_) for _ in range(NL_)]
        self.final_ln = (1.0 + 0.1 * torch.randn(D_, generator=g)).to(BF).to(DEV)
        lm = torch.randn(D_, V_, generator=g) * D_ ** -0.5
        lm[:, EOS_ID] *= eos_scale                                # how often eos is drawn
        self.lm = lm.to(BF).to(DEV)
        self.ref_lm = (lm + 0.02 * torch.randn(D_, V_, generator=g)).to(BF).to(DEV)
        mask = torch.ones(B_, S_, dtype=torch.int64)
        mask[0, 5:] = 0
        mask[2, 3] = 0
        self.mask = mask.to(DEV)
        self.table = P.t5_relative_bias_table(torch.randn(32, NH_, generator=g).to(DEV), T_)
        self.u = torch.rand(T_, B_, generator=g).to(DEV)
        self.kw = dict(temperature=0.9, top_k=10, top_p=0.95)

    def state(self):
        clock = P.T5DecodeClock(T_, DEV)
        caches = [P.T5DecodeKVCache(B_, NH_, DKV_, T_, BF, DEV) for _ in range(NL_)]
        rec = P.PPORolloutRecorder(B_, T_, DEV, pad_token_id=PAD_ID, eos_token_id=EOS_ID, clock=clock)
        bufs = dict(qkv=torch.empty(B_, 3 * INNER_, dtype=BF, device=DEV), cq=torch.empty(B_, INNER_, dtype=BF, device=DEV),
                    ff=torch.empty(B_, F_, dtype=BF, device=DEV))
        return clock, caches, rec, torch.empty(B_, D_, dtype=BF, device=DEV), bufs

    def step(self, state, skip):
        """One token.  skip False: t5_decode_layer_fused and the attentions as they were.  skip True:
        live=rec.unfinished in the attentions and, with split_rows=True, in the projections."""
        clock, caches, rec, hbuf, bufs = state
        h, _ = P.t5_decode_embed(self.shared, rec, clock, START_ID, out=(hbuf, None))
        akw = dict(live=rec.unfinished) if skip else {}
        lkw = dict(live=rec.unfinished, split_rows=True) if skip else {}
        for i, blk in enumerate(self.blocks):
            P.t5_decode_layer_fused(
                h, blk, lambda q, kn, vn: P.t5_decode_self_attention(q, kn, vn, caches[i], clock, self.table, **akw),
                lambda q: P.t5_decode_cross_attention(q, self.k_enc[i], self.v_enc[i], self.mask, **akw), bufs=bufs, **lkw)
        y = P.t5_rmsnorm(h, self.final_ln)
        P.ppo_sample_step(torch.matmul(y, self.lm), ref_logits=torch.matmul(y, self.ref_lm), recorder=rec,
                          values=y[:, 0].contiguous(), u=self.u, **self.kw)
        clock.advance()


def rollout_precondition(rec):
    """At least two rows finish before the last column and at least two never draw eos: the skip and
    the live path both run until the last step."""
    tokens = rec.tokens.cpu()
    early = [b for b in range(B_) if (tokens[b, :T_ - 1] == EOS_ID).any()]
    late = [b for b in range(B_) if not (tokens[b] == EOS_ID).any()]
    return len(early) >= 2 and len(late) >= 2


@pytest.mark.timeout(300)
def test_one_captured_step_with_the_projection_skip_records_the_eager_rollout():
    dec = TinyFusedDecoder(SEED_, EOS_SCALE_)
    with torch.no_grad():
        eager = dec.state()
        for _ in range(T_):
            dec.step(eager, skip=False)
        torch.cuda.synchronize()
        want = eager[2]
        assert rollout_precondition(want), (want.tokens.cpu(), want.lengths.cpu())
        assert eager[0].t == T_ and eager[0].overrun == 0

        state = dec.state()
        clock, caches, rec, _, _ = state
        dec.step(state, skip=True)                                # warm-up: every lazy initialisation is done
        torch.cuda.synchronize()
        rec.reset()
        for c in caches:
            c.k.zero_()
            c.v.zero_()
        assert clock.t == 0
        scratch = torch.zeros(8, device=DEV)
        try:                                                      # only a missing capture facility may skip
            probe = torch.cuda.CUDAGraph()
            with torch.cuda.graph(probe):
                scratch.add_(1.0)
            probe.replay()
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.skip(f"graph capture is unavailable here: {e}")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                             # one stream, a linear chain of launches
            dec.step(state, skip=True)
        assert clock.t == 0                                       # a capture runs nothing
        for _ in range(T_ + 2):
            graph.replay()
        torch.cuda.synchronize()
    for f in RECORD:
        assert C.same(getattr(rec, f), getattr(want, f)), f
    assert clock.t == T_ and clock.overrun == 2
