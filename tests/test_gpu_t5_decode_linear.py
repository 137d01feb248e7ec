"""trlx_t5_decode_linear on the GPU (csrc/t5_decode_linear.hip; t5_decode_linear.t5_decode_linear): a
decode-step projection with the RMSNorm in front and the residual add or the (gated) activation
behind it, against the kernels and the torch ops it replaces.

Every operand is a strided slice of a larger allocation with guard margins on both sides, so that
even a missing guard in the kernel would stay inside the test's own memory; the margins are checked
afterwards.

Measured on the MI355X, the worst max|kernel - oracle| / (2 max|unfused - oracle| + one bf16 ulp) over
the shapes of t5_decode_linear_checks.shapes, per combination, is recorded in
profiles/t5_decode_linear_parity.json (tools/t5_decode_linear_bench.py --parity writes it)."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_rollout_checks as C
import t5_decode_linear_checks as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
PAD = 8                                         # row stride = columns + PAD: strided rows on the 16-byte grid


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


def eye_rows(K, N):
    """The first N rows of the K x K identity."""
    w = torch.zeros(N, K, dtype=BF, device=DEV)
    w[torch.arange(N), torch.arange(N)] = 1.0
    return w


def anchor_shapes(norm):
    """(M, N, K): the full identity (K = N) at the small sizes, the identity's first 48 rows at both
    sides of every K break."""
    out = [(m, k, k) for m in L.MS for k in L.KS]
    out += [(17, 48, k) for b in L.K_BREAKS for k in (b, b + 32) if not norm or k <= L.NORM_MAX_K]
    out += [(m, 96, 96) for m in L.M_BREAKS]
    return out


def anchor_x(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[0] *= 1e3
    if M > 1:
        x[1] *= 1e-3
    return strided(x.to(BF).to(DEV))


# ------------------------------------------------------------------ exact anchors
@pytest.mark.parametrize("norm", (False, True), ids=("plain", "norm"))
def test_identity_weight_returns_x_or_its_rmsnorm_bit_for_bit(norm):
    for M, N, K in anchor_shapes(norm):
        x_all, x = anchor_x(M, K, 7 * K + M)
        nw = (1.0 + 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(K))).to(BF).to(DEV) if norm else None
        o_all, out = guarded_out(M, N)
        got = P.t5_decode_linear(x, eye_rows(K, N), norm_weight=nw, out=out)
        assert got is out
        want = P.t5_rmsnorm(x, nw) if norm else x
        assert C.same(out.contiguous(), want[:, :N].contiguous()), (M, N, K)
        assert margins_kept(o_all, out) and margins_kept(x_all, x), (M, N, K)


@pytest.mark.parametrize("alias", (False, True), ids=("out", "in_place"))
def test_identity_weight_with_residual_is_torchs_bf16_sum(alias):
    for M, N, K in anchor_shapes(False):
        x_all, x = anchor_x(M, K, 11 * K + M)
        r_all, res = strided(torch.randn(M, N, generator=torch.Generator().manual_seed(K + M)).to(BF).to(DEV))
        want = (x[:, :N] + res).contiguous()
        if alias:
            got = P.t5_decode_linear(x, eye_rows(K, N), residual=res, out=res)
            assert got is res and margins_kept(r_all, res)
        else:
            before = r_all.clone()
            o_all, got = guarded_out(M, N)
            P.t5_decode_linear(x, eye_rows(K, N), residual=res, out=got)
            assert margins_kept(o_all, got) and C.same(r_all, before)
        assert C.same(got.contiguous(), want), (M, N, K)


@pytest.mark.parametrize("gated", (False, True), ids=("act", "gated"))
@pytest.mark.parametrize("act", L.ACTS)
def test_identity_weight_with_activation_is_t5_ff_act_bit_for_bit(act, gated):
    for M, N, K in anchor_shapes(False):
        x_all, x = anchor_x(M, K, 13 * K + M)
        w = eye_rows(K, N)
        o_all, out = guarded_out(M, N)
        P.t5_decode_linear(x, torch.cat([w, w], 0) if gated else w, act=act, gated=gated, out=out)
        xs = x[:, :N]
        want = P.t5_ff_act(xs, xs if gated else None, act)
        assert C.same(out.contiguous(), want), (M, N, K)
        assert margins_kept(o_all, out), (M, N, K)


# ------------------------------------------------------------------ accuracy and determinism
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_accuracy_against_the_float64_oracle_and_two_calls_agree(combo):
    norm, (_, with_res, act, gated) = combo
    worst = 0.0
    for M, N, K in L.shapes(norm):
        x, w, nw, res = L.inputs(M, N, K, gated, seed=1000 * K + 10 * N + M, device=DEV)
        kw = dict(norm_w=nw if norm else None, residual=res if with_res else None, act=act, gated=gated)
        ref = L.oracle(x, w, **kw)
        e_unfused = L.max_err(L.unfused(x, w, **kw), ref)
        (x_all, xs), (w_all, ws), (r_all, rs) = strided(x), strided(w), strided(res)
        before = [t.clone() for t in (x_all, w_all, r_all)]
        fkw = dict(norm_weight=kw["norm_w"], residual=rs if with_res else None, act=act, gated=gated)
        o_all, out = guarded_out(M, N)
        P.t5_decode_linear(xs, ws, out=out, **fkw)
        o2_all, out2 = guarded_out(M, N)
        P.t5_decode_linear(xs, ws, out=out2, **fkw)
        e_kernel = L.max_err(out, ref)
        limit = L.bound(e_unfused, ref)
        print(f"{L.combo_name(combo)} M {M} N {N} K {K}: e_kernel {e_kernel:.4g} e_unfused {e_unfused:.4g} "
              f"bound {limit:.4g} ratio {e_kernel / limit:.3f}")
        worst = max(worst, e_kernel / limit)
        assert torch.isfinite(out.float()).all(), (M, N, K)
        assert e_kernel <= limit, (M, N, K, e_kernel, e_unfused, limit)
        assert C.same(out.contiguous(), out2.contiguous()), (M, N, K, "two calls differ")
        assert margins_kept(o_all, out) and margins_kept(o2_all, out2), (M, N, K)
        assert all(C.same(a, b) for a, b in zip((x_all, w_all, r_all), before)), (M, N, K, "an input was written")
    print(f"{L.combo_name(combo)}: worst ratio {worst:.3f}")


def test_a_3d_decode_slice_and_a_last_position_view_are_read_in_place():
    g = torch.Generator().manual_seed(5)
    hseq = torch.randn(3, 4, 96, generator=g).to(BF).to(DEV)
    w = (torch.randn(48, 96, generator=g) / 96 ** 0.5).to(BF).to(DEV)
    want = P.t5_decode_linear(hseq[:, -1, :].contiguous(), w)
    assert C.same(P.t5_decode_linear(hseq[:, -1, :], w), want)
    got3 = P.t5_decode_linear(hseq[:, -1:, :], w)
    assert got3.shape == (3, 1, 48) and C.same(got3[:, 0, :], want)


def test_fp32_and_off_grid_shapes_take_the_torch_route():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 40, generator=g).to(DEV)
    w = torch.randn(24, 40, generator=g).to(DEV)
    nw = torch.ones(40, device=DEV)
    assert torch.allclose(P.t5_decode_linear(x, w, norm_weight=nw), P.t5_rmsnorm(x, nw) @ w.t())
    xb, wb = x.to(BF), w.to(BF)                   # bf16, K = 40 off the grid
    assert C.same(P.t5_decode_linear(xb, wb), torch.matmul(xb, wb.t()))
    with pytest.raises(ValueError):
        P.t5_decode_linear(xb.requires_grad_(True), wb)


# ------------------------------------------------------------------ refusals
def _args(xt, wt, ot, nw=None, res=None, act=_lib.T5_ACT_NONE, gated=0, dtype=_lib.BF16, **over):
    """The arguments of a valid call on these tensors, then `over` on top of them."""
    M, K = xt.shape
    N = ot.shape[1]
    kw = dict(x=xt.data_ptr(), ld_x=xt.stride(0), weight=wt.data_ptr(), ld_w=wt.stride(0), norm_weight=_lib.ptr(nw),
              residual=_lib.ptr(res), ld_residual=N if res is None else res.stride(0), out=ot.data_ptr(),
              ld_out=ot.stride(0), M=M, K=K, N=N, eps=1e-6, dtype=dtype, act=act, gated=gated)
    kw.update(over)
    return _lib.T5DecodeLinearArgs(**kw)


def test_every_refusal_returns_its_status_and_leaves_out_untouched():
    lib = _lib.load()
    M, N, K = 3, 16, 64
    x, w, nw, res = L.inputs(M, N, K, True, seed=9, device=DEV)
    (_, xs), (_, ws), (_, rs) = strided(x), strided(w), strided(res)
    o_all, out = guarded_out(M, N)
    big = torch.zeros(M, L.NORM_MAX_K + 32, dtype=BF, device=DEV)
    wbig = torch.zeros(N, L.NORM_MAX_K + 32, dtype=BF, device=DEV)
    nwbig = torch.ones(L.NORM_MAX_K + 32, dtype=BF, device=DEV)
    stream = _lib.stream_of(out)
    w1 = ws[:N]
    cases = [
        ("NULL args", None, C.ERR_ARG),
        ("NULL x", _args(xs, w1, out, x=None), C.ERR_ARG),
        ("NULL weight", _args(xs, w1, out, weight=None), C.ERR_ARG),
        ("NULL out", _args(xs, w1, out, out=None), C.ERR_ARG),
        ("fp32", _args(xs, w1, out, dtype=_lib.F32), C.ERR_DTYPE),
        ("M 0", _args(xs, w1, out, M=0), C.ERR_SHAPE),
        ("K not a multiple of 32", _args(xs, w1, out, K=48), C.ERR_SHAPE),
        ("K 0", _args(xs, w1, out, K=0), C.ERR_SHAPE),
        ("K above 16384", _args(xs, w1, out, K=16416, ld_x=16424, ld_w=16424), C.ERR_SHAPE),
        ("N not a multiple of 16", _args(xs, w1, out, N=8), C.ERR_SHAPE),
        ("K above 8192 with a norm weight", _args(big, wbig, out, nw=nwbig), C.ERR_SHAPE),
        ("x off 16 bytes", _args(xs, w1, out, x=xs.data_ptr() + 2), C.ERR_ARG),
        ("weight off 16 bytes", _args(xs, w1, out, weight=w1.data_ptr() + 8), C.ERR_ARG),
        ("out off 16 bytes", _args(xs, w1, out, out=out.data_ptr() + 4), C.ERR_ARG),
        ("norm weight off 16 bytes", _args(xs, w1, out, norm_weight=nw.data_ptr() + 2), C.ERR_ARG),
        ("residual off 16 bytes", _args(xs, w1, out, res=rs, residual=rs.data_ptr() + 2), C.ERR_ARG),
        ("x stride below K", _args(xs, w1, out, ld_x=K - 8), C.ERR_STRIDE),
        ("x stride off the grid", _args(xs, w1, out, ld_x=K + 4), C.ERR_STRIDE),
        ("weight stride off the grid", _args(xs, w1, out, ld_w=K + 2), C.ERR_STRIDE),
        ("out stride below N", _args(xs, w1, out, ld_out=8), C.ERR_STRIDE),
        ("out stride off the grid", _args(xs, w1, out, ld_out=N + 4), C.ERR_STRIDE),
        ("residual stride off the grid", _args(xs, w1, out, res=rs, ld_residual=N + 4), C.ERR_STRIDE),
        ("out overlaps x", _args(xs, w1, out, out=xs.data_ptr(), ld_out=xs.stride(0)), C.ERR_ARG),
        ("out overlaps weight", _args(xs, w1, out, out=w1.data_ptr(), ld_out=w1.stride(0)), C.ERR_ARG),
        ("out overlaps the norm weight", _args(xs, w1, out, nw=nw, out=nw.data_ptr(), M=1, N=16), C.ERR_ARG),
        ("out overlaps residual, shifted", _args(xs, w1, out, res=rs, out=rs.data_ptr() + 16, ld_out=rs.stride(0)), C.ERR_ARG),
        ("out is residual with another stride", _args(xs, w1, out, res=rs, out=rs.data_ptr(), ld_out=rs.stride(0) + 8), C.ERR_ARG),
        ("both epilogues", _args(xs, w1, out, res=rs, act=_lib.T5_ACT_SILU), C.ERR_ARG),
        ("gated without an act", _args(xs, ws, out, gated=1), C.ERR_ARG),
        ("an unknown act", _args(xs, w1, out, act=7), C.ERR_ARG),
        ("eps NaN", _args(xs, w1, out, nw=nw, eps=float("nan")), C.ERR_ARG),
    ]
    snapshot = [t.clone() for t in (xs, ws, rs, nw)]
    for name, a, status in cases:
        rc = lib.trlx_t5_decode_linear(None if a is None else ctypes.byref(a), stream)
        assert rc == status, (name, rc, lib.trlx_last_error())
        assert lib.trlx_last_error(), name
    torch.cuda.synchronize()
    assert C.same(o_all, torch.full_like(o_all, C.GUARD))
    assert all(C.same(a, b) for a, b in zip((xs, ws, rs, nw), snapshot))
    # the python entry refuses before the library is asked
    for bad in (dict(residual=rs, act="silu"), dict(gated=True), dict(act="gelu")):
        with pytest.raises(ValueError):
            P.t5_decode_linear(xs, w1, **bad)


# ------------------------------------------------------------------ one captured 8-launch layer step
B_, D_, NH_, DKV_, F_, S_, T_, V_ = 3, 64, 2, 64, 96, 5, 4, 11
INNER_ = NH_ * DKV_


class Layer:
    """One decoder layer (gated gelu_new) and what a decode step needs around it."""

    def __init__(self):
        sd = L.hf_block_state_dict(D_, INNER_, F_, True, seed=21, device=DEV)
        self.w = P.T5DecodeBlockWeights.from_state_dict(sd, "decoder.block.0.", gated=True)
        g = torch.Generator().manual_seed(22)
        self.shared = torch.randn(V_, D_, generator=g).to(BF).to(DEV)
        self.tokens = torch.randint(0, V_, (B_, T_), generator=g).to(DEV)
        self.table = P.t5_relative_bias_table(torch.randn(32, NH_, generator=g).to(DEV), T_)
        self.k_enc = (torch.randn(B_, NH_, S_, DKV_, generator=g) * DKV_ ** -0.25).to(BF).to(DEV)
        self.v_enc = torch.randn(B_, NH_, S_, DKV_, generator=g).to(BF).to(DEV)
        self.mask = torch.ones(B_, S_, dtype=torch.int64, device=DEV)
        self.mask[1, S_ - 2:] = 0

    def state(self):
        return dict(clock=P.T5DecodeClock(T_, DEV), cache=P.T5DecodeKVCache(B_, NH_, DKV_, T_, BF, DEV),
                    h=torch.zeros(B_, D_, dtype=BF, device=DEV), hs=torch.zeros(T_, B_, D_, dtype=BF, device=DEV),
                    bufs=dict(qkv=torch.empty(B_, 3 * INNER_, dtype=BF, device=DEV),
                              cq=torch.empty(B_, INNER_, dtype=BF, device=DEV), ff=torch.empty(B_, F_, dtype=BF, device=DEV)))

    def step_fused(self, st, t=None):
        """8 launches in the layer; t None: the clock form (the captured step), which also advances."""
        tt = st["clock"] if t is None else t
        P.t5_decode_embed(self.shared, self.tokens, tt, 0, out=(st["h"], None))
        P.t5_decode_layer_fused(st["h"], self.w, lambda q, k, v: P.t5_decode_self_attention(q, k, v, st["cache"], tt, self.table),
                                lambda q: P.t5_decode_cross_attention(q, self.k_enc, self.v_enc, self.mask), bufs=st["bufs"])
        if t is None:
            st["clock"].advance()

    def step_unfused(self, st, t):
        """The 12-launch layer on the same weights (kept as [N, K]: matmul against the transposed view)."""
        w = self.w
        h, y = P.t5_decode_embed(self.shared, self.tokens, t, 0, w.ln[0])
        qkv = torch.matmul(y, w.qkv.t())
        q, kn, vn = (qkv[:, j * INNER_:(j + 1) * INNER_] for j in range(3))
        a = P.t5_decode_self_attention(q, kn, vn, st["cache"], t, self.table)
        h, y = P.t5_add_rmsnorm(torch.matmul(a, w.o.t()), h, w.ln[1])
        c = P.t5_decode_cross_attention(torch.matmul(y, w.cq.t()), self.k_enc, self.v_enc, self.mask)
        h, y = P.t5_add_rmsnorm(torch.matmul(c, w.co.t()), h, w.ln[2])
        f = P.t5_ff_act_packed(torch.matmul(y, w.wi.t()), "gelu_new")
        st["h"].copy_(h + torch.matmul(f, w.wo.t()))


@pytest.mark.timeout(300)
def test_one_captured_layer_step_replays_the_eager_fused_loop_bit_for_bit():
    layer = Layer()
    eager, cap = layer.state(), layer.state()
    with torch.no_grad():
        for t in range(T_):
            layer.step_fused(eager, t)
            eager["hs"][t].copy_(eager["h"])
        layer.step_fused(cap)                                     # warm-up in the clock form
        torch.cuda.synchronize()
        cap["clock"].reset()
        cap["cache"].k.zero_()
        cap["cache"].v.zero_()
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
            layer.step_fused(cap)
        assert cap["clock"].t == 0
        for t in range(T_):
            graph.replay()
            cap["hs"][t].copy_(cap["h"])
        torch.cuda.synchronize()
    assert cap["clock"].t == T_ and cap["clock"].overrun == 0
    assert C.same(cap["hs"], eager["hs"])
    assert C.same(cap["cache"].k, eager["cache"].k) and C.same(cap["cache"].v, eager["cache"].v)
    for n in ("qkv", "cq", "ff"):
        assert C.same(cap["bufs"][n], eager["bufs"][n]), n


def _layer_oracle(layer, t_last):
    """float64 of the whole T-token loop on the bf16 weights and inputs, nothing rounded in between:
    the final step's h."""
    w = layer.w
    d = lambda x: x.double()
    kc = torch.zeros(B_, NH_, T_, DKV_, dtype=torch.float64, device=DEV)
    vc = torch.zeros_like(kc)
    norm = lambda x, g: d(g) * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6))
    h = None
    for t in range(t_last + 1):
        tok = torch.zeros(B_, dtype=torch.int64, device=DEV) if t == 0 else layer.tokens[:, t - 1]
        h = d(layer.shared)[tok]
        qkv = norm(h, w.ln[0]) @ d(w.qkv).t()
        q, kn, vn = (qkv[:, j * INNER_:(j + 1) * INNER_].view(B_, NH_, DKV_) for j in range(3))
        kc[:, :, t], vc[:, :, t] = kn, vn
        s = torch.einsum("bhd,bhjd->bhj", q, kc[:, :, :t + 1]) + d(layer.table)[None, :, :t + 1].flip(-1)
        a = torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), vc[:, :, :t + 1]).reshape(B_, INNER_)
        h = h + a @ d(w.o).t()
        q = (norm(h, w.ln[1]) @ d(w.cq).t()).view(B_, NH_, DKV_)
        s = torch.einsum("bhd,bhjd->bhj", q, d(layer.k_enc)).masked_fill(layer.mask[:, None, :] == 0, float("-inf"))
        c = torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), d(layer.v_enc)).reshape(B_, INNER_)
        h = h + c @ d(w.co).t()
        uv = norm(h, w.ln[2]) @ d(w.wi).t()
        h = h + (L.gelu_new64(uv[:, :F_]) * uv[:, F_:]) @ d(w.wo).t()
    return h


def test_the_8_launch_layer_is_as_close_to_float64_as_the_12_launch_layer():
    layer = Layer()
    fused, plain = layer.state(), layer.state()
    with torch.no_grad():
        for t in range(T_):
            layer.step_fused(fused, t)
            layer.step_unfused(plain, t)
        ref = _layer_oracle(layer, T_ - 1)
    e_fused, e_plain = L.max_err(fused["h"], ref), L.max_err(plain["h"], ref)
    print(f"final h: e_fused {e_fused:.4g} e_12_launch {e_plain:.4g} bound {L.bound(e_plain, ref):.4g}")
    assert e_fused <= L.bound(e_plain, ref), (e_fused, e_plain)
