"""The T5 feed-forward activation on the device: trlx_t5_ff_act_fwd / _bwd, t5_ff_act,
t5_ff_act_packed and T5FeedForward.

Parity is per element under the rule of t5_ff_act_checks (|got - ref| <= ulp(|ref|) + 2^-16 M
against the float64 oracle), for both dtypes, the three activations, gated and not, at sizes taken
from trlx_t5_ff_act_geometry, forward and backward, the tail row included.  What no tolerance can
hide is checked in bits: layouts against the contiguous call, the two access forms, run-to-run,
canaries, refusals.  TRLX_T5_FF_ACT_PARITY_OUT=<file> writes the measured figures: per case the
kernel's worst ratio to the rule and HF's eager op sequence's (on the elements after the tail
values: HF's own backward gives 0 * inf on those)."""
import ctypes
import json
import os

import pytest
import torch
from transformers import T5Config
from transformers.models.t5.modeling_t5 import T5DenseActDense, T5DenseGatedActDense

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_ff_act_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = 77.0
FIGURES = []
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def geometry():
    t = [ctypes.c_int(0) for _ in range(4)]
    _lib.call("trlx_t5_ff_act_geometry", *[ctypes.byref(x) for x in t])
    return [x.value for x in t]


def sizes(dtype):
    vb, vf, cols, rows = geometry()
    vec = vb if dtype == torch.bfloat16 else vf
    Fs = [1, vec - 1, vec, vec + 1, cols - 1, cols + 1, 2 * cols + vec + 3]
    Ns = [1, rows + 1, 3 * rows + 2]
    return vec, cols, rows, Fs, Ns


@pytest.fixture(scope="module", autouse=True)
def figures_file():
    yield
    path = os.environ.get("TRLX_T5_FF_ACT_PARITY_OUT")
    if path and FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "|got - ref| <= ulp_dtype(|ref|) + 2^-16 * M per element against the float64 oracle; "
                               "figures are the worst ratio to that bound over the case's elements and outputs",
                       "geometry": dict(zip(("vec_bf16", "vec_f32", "cols_per_block", "rows_per_block"), geometry())),
                       "cases": FIGURES}, f, indent=1)


# ------------------------------------------------------------------ operands in canaried buffers
def place(x, ld=None, col0=0):
    """x [N, F] as rows 1..N, columns col0..col0+F of a canaried [N + 2, ld] buffer: (buffer, view)."""
    N, F = x.shape
    buf = torch.full((N + 2, ld or F), CANARY, dtype=x.dtype, device=DEV)
    view = buf[1:N + 1, col0:col0 + F]
    view.copy_(x)
    return buf, view


def blank(N, F, dtype, ld=None, col0=0):
    buf = torch.full((N + 2, ld or F), CANARY, dtype=dtype, device=DEV)
    return buf, buf[1:N + 1, col0:col0 + F]


def intact(buf, view):
    """Every element of buf outside view still holds the canary."""
    keep = torch.ones_like(buf, dtype=torch.bool)
    r0 = (view.data_ptr() - buf.data_ptr()) // buf.element_size() // buf.stride(0)
    c0 = (view.data_ptr() - buf.data_ptr()) // buf.element_size() % buf.stride(0)
    keep[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    return bool((buf[keep] == CANARY).all())


def args_of(act, dtype, N, F, **ops):
    kw = {}
    for name in ("u", "v", "out", "dy", "du", "dv"):
        t = ops.get(name)
        kw[name] = None if t is None else t.data_ptr()
        kw[f"ld_{name}"] = F if t is None else t.stride(0)
    return _lib.T5FfActArgs(N=N, F=F, dtype=_lib.BF16 if dtype == torch.bfloat16 else _lib.F32, act=P.t5_ff.ACTS[act], **kw)


def call(entry, act, dtype, N, F, **ops):
    _lib.call(entry, ctypes.byref(args_of(act, dtype, N, F, **ops)), _lib.stream_of(ops["u"]))


def run(c, act, layout="contig", vec=8):
    """Forward and backward of one case in a layout; {"y", "du", "dv"} as contiguous copies, after
    checking every canary.  Layouts: contig, strided (ld = F + vec), odd (ld = F + 3), col1 (a view
    that starts at column 1), packed (u | v and du | dv as the halves of one [N, 2F] tensor each)."""
    u, v, dy = c["u"], c["v"], c["dy"]
    N, F = u.shape
    dt = u.dtype
    ld, col0 = {"contig": (F, 0), "strided": (F + vec, 0), "odd": (F + 3, 0), "col1": (F + vec, 1), "packed": (F, 0)}[layout]
    bufs = []

    def inp(x):
        b, w = place(x, ld, col0)
        bufs.append((b, w))
        return w

    def outp():
        b, w = blank(N, F, dt, ld, col0)
        bufs.append((b, w))
        return w

    if layout == "packed":
        assert v is not None
        b, w = place(torch.cat([u, v], dim=1))
        bufs.append((b, w))
        ud, vd = w[:, :F], w[:, F:]
        b, w = blank(N, 2 * F, dt)
        bufs.append((b, w))
        du, dvw = w[:, :F], w[:, F:]
    else:
        ud, vd = inp(u), None if v is None else inp(v)
        du, dvw = outp(), None if v is None else outp()
    dyd, out = inp(dy), outp()
    call("trlx_t5_ff_act_fwd", act, dt, N, F, u=ud, v=vd, out=out)
    call("trlx_t5_ff_act_bwd", act, dt, N, F, u=ud, v=vd, dy=dyd, du=du, dv=dvw)
    torch.cuda.synchronize()
    for b, w in bufs:
        assert intact(b, w), (layout, N, F)
    got = {"y": out.contiguous(), "du": du.contiguous()}
    if v is not None:
        got["dv"] = dvw.contiguous()
    return got


def on_device(c):
    return {k: (None if t is None else t.to(DEV)) for k, t in c.items()}


# ------------------------------------------------------------------ parity, layouts, canaries
@pytest.mark.parametrize("gated", [True, False], ids=["gated", "ungated"])
@pytest.mark.parametrize("act", C.ACTS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_parity_layouts_and_canaries(dt, act, gated):
    dtype = DTYPES[dt]
    vec, cols, rows, Fs, Ns = sizes(dtype)
    for i, (F, N) in enumerate((F, N) for F in Fs for N in Ns):
        scale = (1.0, 3.0)[i % 2]
        c = C.case(N, F, dtype, scale=scale, gated=gated, seed=i)
        want = C.oracle(c["u"], c["v"], c["dy"], act)
        d = on_device(c)
        got = run(d, act, "contig", vec)
        figs = C.judge(got, want, c["u"], c["v"], c["dy"], dtype)
        tail = min(len(C.TAIL), N * F)
        hf = None
        if N * F > tail:
            e = C.eager(d["u"], d["v"], d["dy"], act)
            cut = lambda t: None if t is None else t.reshape(-1)[tail:]
            hf = C.judge({n: cut(t) for n, t in e.items()}, {n: cut(t) for n, t in want.items()},
                         cut(c["u"]), cut(c["v"]), cut(c["dy"]), dtype)
        FIGURES.append(dict(dtype=dt, act=act, gated=gated, N=N, F=F, scale=scale, kernel=figs,
                            kernel_worst=max(figs.values()), hf_eager=hf, hf_eager_worst=None if hf is None else max(hf.values())))
        print(dt, act, gated, N, F, figs, hf)
        assert set(figs) == ({"y", "du", "dv"} if gated else {"y", "du"})
        for n, r in figs.items():
            assert bool(torch.isfinite(got[n]).all()), (n, N, F)          # the inputs are all finite
            assert r <= 1.0, (n, N, F, figs)
        # the other layouts give the contiguous call's bits; F a multiple of vec keeps the 16-byte
        # form under "strided", everything else ("odd" row strides, a view from column 1) takes the
        # element form
        for layout in ("strided", "odd", "col1") + (("packed",) if gated else ()):
            other = run(d, act, layout, vec)
            for n in got:
                assert torch.equal(other[n], got[n]), (layout, n, N, F)


@pytest.mark.parametrize("gated", [True, False], ids=["gated", "ungated"])
@pytest.mark.parametrize("act", C.ACTS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_nan_stays_in_its_element_and_runs_repeat(dt, act, gated):
    dtype = DTYPES[dt]
    vec, cols, rows, Fs, Ns = sizes(dtype)
    N, F = rows + 1, cols + vec
    c = C.case(N, F, dtype, scale=3.0, gated=gated, seed=99)
    first = run(on_device(c), act, "contig", vec)
    again = run(on_device(c), act, "contig", vec)
    for n in first:
        assert torch.equal(first[n], again[n]), n
    for where in ((0, 0), (rows, cols + 1), (3, 100)):
        c2 = dict(c, u=c["u"].clone())
        c2["u"][where] = float("nan")
        for layout in ("contig", "col1"):
            got = run(on_device(c2), act, layout, vec)
            for n, t in got.items():
                bad = torch.isnan(t)
                assert bool(bad[where]) and int(bad.sum()) == 1, (n, where, layout)
                t = t.clone()
                t[where] = first[n][where]
                assert torch.equal(t, first[n]), (n, where, layout)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched_and_n0_succeeds():
    dtype, act, N, F = torch.bfloat16, "gelu_new", 5, 24
    c = on_device(C.case(N, F, dtype))
    ub, u = place(c["u"], F + 8)
    vb, v = place(c["v"], F + 8)
    gb, dy = place(c["dy"], F + 8)
    ob, out = blank(N, F, dtype, F + 8)
    dub, du = blank(N, F, dtype, F + 8)
    dvb, dv = blank(N, F, dtype, F + 8)
    pk, pw = blank(N, 2 * F, dtype)                      # a packed gradient: halves are fine, shifted halves are not
    fwd = dict(u=u, v=v, out=out)
    bwd = dict(u=u, v=v, dy=dy, du=du, dv=dv)

    def refused(entry, ops, N_=N, F_=F, act_=act, code=None, **patch):
        a = args_of(act_, dtype, N_, F_, **ops)
        for k, val in patch.items():
            setattr(a, k, val)
        if code is not None:
            a.dtype = code
        with pytest.raises(ValueError):
            _lib.call(entry, ctypes.byref(a), _lib.stream_of(u))

    for name in ("u", "out"):
        refused("trlx_t5_ff_act_fwd", fwd, **{name: None})
    for name in ("u", "dy"):
        refused("trlx_t5_ff_act_bwd", bwd, **{name: None})
    refused("trlx_t5_ff_act_bwd", bwd, du=None, dv=None)
    refused("trlx_t5_ff_act_bwd", bwd, v=None)                        # dv asked for with no v
    for entry, ops in (("trlx_t5_ff_act_fwd", fwd), ("trlx_t5_ff_act_bwd", bwd)):
        refused(entry, ops, F_=0)
        refused(entry, ops, F_=-3)
        refused(entry, ops, N_=-1)
        refused(entry, ops, code=_lib.I64)
        refused(entry, ops, code=7)
        refused(entry, ops, act=3)
        refused(entry, ops, act=-1)
        for name in ops:
            refused(entry, ops, **{f"ld_{name}": F - 1})
    # a written operand that shares an element with another operand
    refused("trlx_t5_ff_act_fwd", dict(u=u, v=v, out=u))
    refused("trlx_t5_ff_act_fwd", dict(u=u, v=v, out=v))
    refused("trlx_t5_ff_act_fwd", dict(u=u, v=v, out=ub[1:N + 1, 4:4 + F]))            # same rows, shifted 4 columns
    refused("trlx_t5_ff_act_fwd", dict(u=u, v=v, out=ub[0:N, 0:F]))                    # a row up: ranges interleave, rows meet
    refused("trlx_t5_ff_act_fwd", dict(u=pw[:, :F], v=pw[:, F:], out=pw[:, F // 2:F // 2 + F]))
    refused("trlx_t5_ff_act_bwd", dict(bwd, du=dy))
    refused("trlx_t5_ff_act_bwd", dict(bwd, dv=du))
    refused("trlx_t5_ff_act_bwd", dict(bwd, du=pw[:, :F], dv=pw[:, F - 1:2 * F - 1]))
    skew = torch.as_strided(pk, (N, F), (2 * F - 2, 1), pw.storage_offset() + F)       # interleaved, unequal row strides
    refused("trlx_t5_ff_act_bwd", dict(bwd, du=pw[:, :F], dv=skew))
    torch.cuda.synchronize()
    for b, w in ((ob, out), (dub, du), (dvb, dv), (pk, pw)):
        assert bool((b == CANARY).all())
    for b, w, x in ((ub, u, c["u"]), (vb, v, c["v"]), (gb, dy, c["dy"])):
        assert intact(b, w) and torch.equal(w, x)
    # N == 0: success, no launch, nothing written (the pointers may be anything non-null)
    call("trlx_t5_ff_act_fwd", act, dtype, 0, F, **fwd)
    call("trlx_t5_ff_act_bwd", act, dtype, 0, F, **bwd)
    torch.cuda.synchronize()
    for b in (ob, dub, dvb):
        assert bool((b == CANARY).all())
    assert P.t5_ff_act(torch.empty(0, F, dtype=dtype, device=DEV), torch.empty(0, F, dtype=dtype, device=DEV)).shape == (0, F)


# ------------------------------------------------------------------ autograd
def _storage(t):
    return t.untyped_storage().data_ptr()


@pytest.mark.parametrize("act,gated", [("gelu_new", True), ("silu", True), ("relu", False)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_autograd_meets_the_rule_and_saves_only_its_inputs(dt, act, gated):
    dtype = DTYPES[dt]
    vec, cols, rows, Fs, Ns = sizes(dtype)
    B, S, F = 3, rows + 1, cols + vec
    c = C.case(B * S, F, dtype, scale=3.0, gated=gated, seed=5)
    want = C.oracle(c["u"], c["v"], c["dy"], act)
    d = on_device(c)
    dy = d["dy"].view(B, S, F)
    u = d["u"].view(B, S, F).clone().requires_grad_()
    v = d["v"].view(B, S, F).clone().requires_grad_() if gated else None
    y = P.t5_ff_act(u, v, act)
    assert y.shape == (B, S, F) and y.is_contiguous()
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert len(saved) == (2 if gated else 1)
    assert _storage(saved[0]) == _storage(u) and saved[0].shape == u.shape
    if gated:
        assert _storage(saved[1]) == _storage(v) and saved[1].shape == v.shape
    grads = torch.autograd.grad(y, [u, v] if gated else [u], dy)
    got = dict(zip(("du", "dv"), (g.reshape(B * S, F) for g in grads)), y=y.detach().reshape(B * S, F))
    figs = C.judge(got, want, c["u"], c["v"], c["dy"], dtype)
    assert set(figs) == ({"y", "du", "dv"} if gated else {"y", "du"})
    assert max(figs.values()) <= 1.0, figs
    if not gated:
        return
    # packed: the same bits, one saved tensor (uv itself), one gradient of uv's shape
    uv = torch.cat([d["u"], d["v"]], dim=1).view(B, S, 2 * F).clone().requires_grad_()
    yp = P.t5_ff_act_packed(uv, act)
    assert torch.equal(yp, y)
    saved = [t for t in yp.grad_fn.saved_tensors if t is not None]
    assert len(saved) == 1 and _storage(saved[0]) == _storage(uv) and saved[0].shape == uv.shape
    (guv,) = torch.autograd.grad(yp, [uv], dy)
    assert guv.shape == uv.shape
    assert torch.equal(guv[..., :F], grads[0]) and torch.equal(guv[..., F:], grads[1])
    # slices of a packed tensor are read in place by the separate call too: the same bits
    ys = P.t5_ff_act(uv[..., :F], uv[..., F:], act)
    assert torch.equal(ys, y)
    saved = [t for t in ys.grad_fn.saved_tensors if t is not None]
    assert [_storage(t) for t in saved] == [_storage(uv)] * 2
    (gs,) = torch.autograd.grad(ys, [uv], dy)
    assert torch.equal(gs, guv)


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del keep
    return rise


def test_a_gradient_that_is_not_needed_is_not_allocated():
    N, F, dtype = 256, 2048, torch.bfloat16
    g = torch.Generator().manual_seed(3)
    u0, v0, dy = (torch.randn(N, F, generator=g).to(dtype).to(DEV) for _ in range(3))
    nbytes = N * F * 2

    want = C.oracle(u0.cpu(), v0.cpu(), dy.cpu(), "gelu_new")
    M = C.factors(u0.cpu(), v0.cpu(), dy.cpu())

    def backward(v_grad):
        u = u0.clone().requires_grad_()
        v = v0.clone().requires_grad_(v_grad)
        y = P.t5_ff_act(u, v, "gelu_new")
        got = {}
        rise = _peak_rise(lambda: got.setdefault("g", torch.autograd.grad(y, [u, v] if v_grad else [u], dy)))
        for n, g in zip(("du", "dv"), got["g"]):
            assert C.ratio(g, want[n], M[n], dtype) <= 1.0, (n, v_grad)
        return rise, got["g"][0]

    both, du_both = backward(True)
    only_du, du_alone = backward(False)
    assert torch.equal(du_both, du_alone)
    assert both == 2 * nbytes and only_du == nbytes, (both, only_du)
    # and the other way round: u frozen, v trained
    u, v = u0.clone(), v0.clone().requires_grad_()
    y = P.t5_ff_act(u, v, "gelu_new")
    only_dv = _peak_rise(lambda: torch.autograd.grad(y, [v], dy))
    assert only_dv == nbytes
    (gv,) = torch.autograd.grad(P.t5_ff_act(u, v, "gelu_new"), [v], dy)
    assert C.ratio(gv, want["dv"], M["dv"], dtype) <= 1.0


def test_forward_and_backward_hold_less_memory_than_hf_eager():
    N, F, dtype = 4096, 2048, torch.bfloat16
    g = torch.Generator().manual_seed(4)
    u0, v0, dy = (torch.randn(N, F, generator=g).to(dtype).to(DEV) for _ in range(3))

    def step(fn):
        u, v = u0.clone().requires_grad_(), v0.clone().requires_grad_()

        def both():
            y = fn(u, v)
            return y, torch.autograd.grad(y, [u, v], dy)

        return _peak_rise(both)

    fused = step(lambda u, v: P.t5_ff_act(u, v, "gelu_new"))
    eager = step(lambda u, v: C.eager_act(u, "gelu_new") * v)
    FIGURES.append(dict(memory=dict(N=N, F=F, dtype="bf16", act="gelu_new", fused_peak_rise_bytes=fused,
                                    hf_eager_peak_rise_bytes=eager, tensor_bytes=N * F * 2)))
    print("peak rise over forward + backward: fused", fused, "HF eager", eager)
    assert fused == 3 * N * F * 2          # y, du, dv and nothing else
    assert fused < eager


# ------------------------------------------------------------------ the module
FORMS = {"gated-gelu": T5DenseGatedActDense, "gated-silu": T5DenseGatedActDense, "relu": T5DenseActDense}


def _bf16_ulp(x):
    return float(C.ulp(torch.tensor([x], dtype=torch.float64), torch.bfloat16))


@pytest.mark.parametrize("proj", list(FORMS))
def test_module_against_hf(proj):
    """Output, input gradient and weight gradients under the project's GEMM-class rule
    e <= 2 e_torch + one bf16 ulp of max|ref|: ref is the HF module in float64 on the bf16 weights
    and inputs, e_torch the error of HF's bf16 module on the device."""
    _, _, cols, _ = geometry()
    cfg = T5Config(d_model=64, d_ff=2 * cols + 8 + 3, feed_forward_proj=proj, dropout_rate=0.0)
    torch.manual_seed(11)
    hf = FORMS[proj](cfg).to(torch.bfloat16).eval()
    x = torch.randn(37, 64, generator=torch.Generator().manual_seed(12)).to(torch.bfloat16)
    g = torch.randn(37, 64, generator=torch.Generator().manual_seed(13)).to(torch.bfloat16)

    def run_module(m, xin, gin):
        xin = xin.clone().requires_grad_()
        y = m(xin)
        y.backward(gin)
        out = {"out": y.detach(), "dx": xin.grad}
        out.update({n: p.grad for n, p in m.named_parameters()})
        return out

    ref_m = FORMS[proj](cfg).double()
    ref_m.load_state_dict({k: t.double() for k, t in hf.state_dict().items()}, strict=True)
    ref = run_module(ref_m, x.double(), g.double())
    mine = P.T5FeedForward(cfg).to(torch.bfloat16)
    mine.load_state_dict(hf.state_dict(), strict=True)
    got = run_module(mine.to(DEV), x.to(DEV), g.to(DEV))
    yard = run_module(hf.to(DEV), x.to(DEV), g.to(DEV))
    assert set(got) == set(ref) == set(yard)
    for n, r in ref.items():
        e_k = float((got[n].double().cpu() - r).abs().max())
        e_t = float((yard[n].double().cpu() - r).abs().max())
        lim = 2.0 * e_t + _bf16_ulp(float(r.abs().max()))
        FIGURES.append(dict(module=proj, tensor=n, e_kernel=e_k, e_torch=e_t, bound=lim))
        print(proj, n, e_k, e_t, lim)
        assert e_k <= lim, (proj, n, e_k, e_t, lim)
