"""The fused lm_head loss side (csrc/lmhead_loss.hip through lm_head.py) around its well-pinned
core (contiguous fp32 operands, tests/test_gpu_lmhead_loss.py): the corners of the drop-in
pair's ABI, and the state that must survive from a forward to its backward.

  B1  row strides: hidden / weight as column slices of wider buffers (NaN padding), dh / dW
      written into wider buffers whose padding must stay untouched; strides the entries refuse;
  B2  the default dtypes: bf16 lp, a bf16 incoming gradient;
  B3  a mask: the compaction (order, live count, compact index of P, the records and the
      scaled rows) under the halves checks, not a Frobenius norm;
  A1  the tuning changed between a forward and its backward: the backward honours the plan its
      forward ran with (the plan token of trlx_lmhead_logprobs_fwd_ex2 / _bwd_ex2);
  A2  the mask edited between forward and backward: refused (an int64 mask kept by reference)
      or without effect (any other mask: a private copy);
  A3  a float mask: live where mask != 0, fractional weights included.

Truth is always lmloss_checks.fp64_truth on the bf16 operands (with a mask: on the live rows
alone), the limits are lmloss_checks.LIMITS, lp and lse at the suite's rtol 1e-5 / 1e-6 with
atol 2e-5.  Shapes are the smallest that are off the 64-token block, the 32-row P tile and the
vocab tiles and still give every vocab split some rows.
"""
import functools

import pytest
import torch

import lmloss_checks as C
import trlx_t5_amd as P
from test_gpu_lmhead_loss import _fwd_saved_bwd, _operands

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
L = P._lib
SHAPES = [(130, 768, 4099), (77, 512, 1031)]
PLANS = ["saved_p", "recompute"]
SPLIT_SHAPE = (200, 768, 7000)  # as test_lm_head_logprobs_split_plans: rows for up to 8 splits
BF16, F32 = torch.bfloat16, torch.float32


@functools.lru_cache(maxsize=None)
def _case(N, H, V):
    """bf16 operands, labels and an upstream gradient on the device (read-only, shared)."""
    h, w, y = _operands(N, H, V, N + V)
    gout = torch.randn(N, generator=torch.Generator().manual_seed(7))
    return h.to(DEV), w.to(DEV), y.to(DEV), gout.to(DEV)


@functools.lru_cache(maxsize=None)
def _mask(N, kind):
    """"some": ~55 % live, the first and the last token masked; "one": a single live token."""
    if kind == "one":
        m = torch.zeros(N, dtype=torch.bool)
        m[N // 2] = True
    else:
        m = torch.rand(N, generator=torch.Generator().manual_seed(N)) < 0.55
        m[0] = m[N - 1] = False
        m[1] = True
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _truth(N, H, V, mask_kind=None, bf16_gout=False):
    """fp64 truth of _case(N, H, V) (the live rows alone under a mask; the upstream gradient
    rounded to bf16 first where the kernels receive it as bf16), computed once."""
    h, w, y, gout = _case(N, H, V)
    if bf16_gout:
        gout = gout.bfloat16().float()
    if mask_kind is not None:
        live = _mask(N, mask_kind)
        h, y, gout = h[live], y[live], gout[live]
    t = C.fp64_truth(h, w, y, gout)
    t["y"], t["g"] = y, gout
    return t


def _check(what, t, dh, dw, e=None, lp=None, lse=None, live=None):
    """lp / lse at the suite's tolerances and the halves checks of E, dh, dW against truth t;
    live: the mask (dh, E, lp, lse rows compared on the live tokens, exact zeros elsewhere)."""
    assert torch.isfinite(dh.float()).all() and torch.isfinite(dw.float()).all(), what
    if live is not None:
        dead = ~live
        assert (dh[dead] == 0).all(), what
        for z in (lp, lse):
            if z is not None:
                assert (z[dead] == 0).all(), what
        dh, e, lp, lse = (None if x is None else x[live] for x in (dh, e, lp, lse))
    if lp is not None:
        torch.testing.assert_close(lp.double(), t["lp"], rtol=1e-5, atol=2e-5)
    if lse is not None:
        torch.testing.assert_close(lse.double(), t["lse"], rtol=1e-6, atol=2e-5)
    errs = C.dw_errors(dw, t["dw"], t["y"])
    errs.update(C.dh_errors(dh, t["dh"], t["g"], t["e"], fp32_out=dh.dtype == F32))
    if e is not None:
        errs.update(C.e_errors(e, t["e"]))
    C.assert_within(errs, what)


def _autograd(h, w, y, gout, plan, mask=None, out_dtype=F32, fwd_knobs=None, bwd_knobs=None, between=None):
    """lm_head_logprobs + backward of Σ gout·lp; returns lp, the node's saved lse and E, dh, dW.
    fwd_knobs / bwd_knobs: tuning held around the forward / the backward only; between: called
    after the forward, before the backward."""
    hg = h.detach().requires_grad_(True)
    wg = w.detach().requires_grad_(True)
    with L.tuning(**(fwd_knobs or {})):
        lp = P.lm_head_logprobs(hg, wg, y, out_dtype=out_dtype, plan=plan, mask=mask)
    saved = lp.grad_fn.saved_tensors
    lse, e = saved[3].clone(), saved[4].clone()
    del saved
    if between is not None:
        between()
    with L.tuning(**(bwd_knobs or {})):
        (lp * gout.to(lp.dtype)).sum().backward()
    torch.cuda.synchronize()
    return lp.detach(), lse, e, hg.grad, wg.grad


# ------------------------------------------------------------------ B1: row strides
def _strided(h, w):
    """hidden as columns [8, 8 + H) of an [N, H + 72] buffer, weight as columns [0, H) of a
    [V, H + 8] one: 16-byte-aligned starts, row strides that are multiples of 8, NaN padding."""
    (N, H), V = h.shape, w.shape[0]
    hb = torch.full((N, H + 72), float("nan"), dtype=BF16, device=DEV)
    wb = torch.full((V, H + 8), float("nan"), dtype=BF16, device=DEV)
    hb[:, 8:8 + H] = h
    wb[:, :H] = w
    return hb[:, 8:8 + H], wb[:, :H]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("N,H,V", SHAPES)
def test_strided_operands_autograd(N, H, V, plan):
    h, w, y, gout = _case(N, H, V)
    hv, wv = _strided(h, w)
    # the call passes these views through as they are (no .contiguous() copy)
    ho, wo, _ = P.lm_head._operands(hv, wv, y)
    assert ho.stride(0) == H + 72 and wo.stride(0) == H + 8 and ho.data_ptr() == hv.data_ptr()
    lp, lse, e, dh, dw = _autograd(hv, wv, y, gout, plan)
    assert dh.shape == (N, H) and dw.shape == (V, H)
    _check(f"strided autograd N={N} V={V} {plan}", _truth(N, H, V), dh, dw, e, lp, lse)


@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("N,H,V", SHAPES)
def test_strided_operands_and_gradients_c_abi(N, H, V, plan, out_dtype):
    """ldh = H + 72, ldw = H + 8, and dh / dW into [N, H + 4] / [V, H + 4] buffers (lddh % 4 == 0
    is the entry's condition): the halves checks, and the gradients' padding bit-unchanged."""
    h, w, y, gout = _case(N, H, V)
    hv, wv = _strided(h, w)
    fill = -7.25  # exact in bf16 and fp32
    lp, lse, e, dh, dw = _fwd_saved_bwd(hv, wv, y, gout, out_dtype, out_dtype, plan, lddh=H + 4, lddw=H + 4,
                                        pad_fill=fill)
    assert dh.stride(0) == H + 4 and dw.stride(0) == H + 4
    _check(f"strided C ABI N={N} V={V} {plan} {out_dtype}", _truth(N, H, V), dh, dw, e, lp, lse)
    assert (dh._base[:, H:] == fill).all() and (dw._base[:, H:] == fill).all()


@pytest.mark.parametrize("which", ["hidden", "weight"])
def test_stride_not_a_multiple_of_8_refused_before_any_launch(which):
    """A row stride of H + 4 elements (8-byte rows) for hidden or weight: TRLX_ERR_STRIDE from
    both entries (ll_check runs first in ll_setup, ahead of the compaction and every kernel), and
    no output is touched."""
    N, H, V = SHAPES[1]
    h, w, y, gout = _case(N, H, V)
    if which == "hidden":
        hb = torch.zeros((N, H + 4), dtype=BF16, device=DEV)
        hb[:, :H] = h
        h = hb[:, :H]
    else:
        wb = torch.zeros((V, H + 4), dtype=BF16, device=DEV)
        wb[:, :H] = w
        w = wb[:, :H]
    fill = 123.0
    f32 = dict(dtype=F32, device=DEV)
    lp, lse, e = torch.full((N,), fill, **f32), torch.full((N,), fill, **f32), torch.full((N, H), fill, **f32)
    dh, dw = torch.full((N, H), fill, **f32), torch.full((V, H), fill, **f32)
    ws = torch.empty(L.query("trlx_lmhead_loss_workspace_bytes", N, H, V), dtype=torch.uint8, device=DEV)
    saved = torch.empty(L.query("trlx_lmhead_savep_bytes", N, H, V), dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream
    with pytest.raises(ValueError, match=r"status 2"):
        L.call("trlx_lmhead_logprobs_fwd_ex", h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), N, H, V,
               y.data_ptr(), 1, None, lp.data_ptr(), L.F32, lse.data_ptr(), e.data_ptr(), ws.data_ptr(),
               saved.data_ptr(), s)
    with pytest.raises(ValueError, match=r"status 2"):
        L.call("trlx_lmhead_logprobs_bwd_ex", h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), N, H, V,
               y.data_ptr(), 1, None, gout.data_ptr(), L.F32, lse.data_ptr(), e.data_ptr(), dh.data_ptr(), H, L.F32,
               dw.data_ptr(), L.F32, H, ws.data_ptr(), saved.data_ptr(), s)
    torch.cuda.synchronize()
    for t in (lp, lse, e, dh, dw):
        assert (t == fill).all()


# ------------------------------------------------------------------ B2: the default dtypes
def _check_bf16_lp(lp, t):
    """One bf16 rounding of lp (relative 2^-9) at twice its bound, on top of the fp32 path's atol."""
    assert lp.dtype == BF16
    err = (lp.double() - t["lp"]).abs()
    bound = 2.0 ** -8 * t["lp"].abs() + 2e-5
    assert (err <= bound).all(), float((err - bound).max())


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("N,H,V", SHAPES)
def test_default_dtypes_autograd(N, H, V, plan):
    """lm_head_logprobs(h, w, y) as a caller gets it by default: lp in hidden's dtype (bf16), so
    autograd hands the backward a bf16 gradient."""
    h, w, y, gout = _case(N, H, V)
    t = _truth(N, H, V, bf16_gout=True)
    lp, lse, e, dh, dw = _autograd(h, w, y, gout.bfloat16(), plan, out_dtype=None)
    _check_bf16_lp(lp, t)
    assert dh.dtype == BF16 and dw.dtype == BF16
    _check(f"default dtypes N={N} V={V} {plan}", t, dh, dw, e, None, lse)


@pytest.mark.parametrize("plan", PLANS)
def test_default_dtypes_c_abi(plan):
    N, H, V = SHAPES[0]
    h, w, y, gout = _case(N, H, V)
    t = _truth(N, H, V, bf16_gout=True)
    lp, lse, e, dh, dw = _fwd_saved_bwd(h, w, y, gout, BF16, BF16, plan, grad_dtype=BF16, lp_dtype=BF16)
    _check_bf16_lp(lp, t)
    _check(f"bf16 lp / grad C ABI {plan}", t, dh, dw, e, None, lse)


# ------------------------------------------------------------------ B3: masked halves
def _masked_inputs(N, H, V, kind):
    """The case's operands with the masked tokens' hidden rows NaN and their labels out of range
    (−100 and V in turn).  k_lmloss_combine returns for a masked token before it reads the
    label (the forward and the backward mode alike) and the MFMA passes index the live tokens
    only, so neither is ever dereferenced."""
    h, w, y, gout = _case(N, H, V)
    live = _mask(N, kind)
    dead = ~live
    hp = h.masked_fill(dead[:, None], float("nan"))
    bad = torch.where(torch.arange(N, device=DEV) % 2 == 0, torch.tensor(-100, device=DEV), torch.tensor(V, device=DEV))
    yp = torch.where(dead, bad, y)
    return hp, w, yp, gout, live


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("kind", ["some", "one"])
@pytest.mark.parametrize("N,H,V", SHAPES)
def test_masked_halves(N, H, V, kind, plan):
    h, w, y, gout, live = _masked_inputs(N, H, V, kind)
    t = _truth(N, H, V, mask_kind=kind)
    what = f"masked ({kind}) N={N} V={V} {plan}"
    lp, lse, e, dh, dw = _autograd(h, w, y, gout, plan, mask=live.long())
    _check(what + " autograd", t, dh, dw, e, lp, lse, live=live)
    for dt in (F32, BF16):  # E is the C ABI's output; fp32 gradients see E through dh as well
        lp, lse, e, dh, dw = _fwd_saved_bwd(h, w, y, gout, dt, dt, plan, mask=live.long())
        _check(what + f" C ABI {dt}", t, dh, dw, e, lp, lse, live=live)


# ------------------------------------------------------------------ A1: tuning changed in between
# (forward knobs, backward knobs): the forward's values held over both halves are the reference
KNOB_CHANGES = [(dict(lmloss_splits=3), dict()), (dict(), dict(lmloss_splits=5)),
                (dict(lmloss_dwp_form=1), dict()), (dict(), dict(lmloss_dw=1))]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("fwd_knobs,bwd_knobs", KNOB_CHANGES)
def test_backward_honours_its_forwards_plan(fwd_knobs, bwd_knobs, masked):
    """The saved-P plan with a tuning knob that differs between the forward and the backward:
    the P tiles and the per-(split, token) records are laid out by the forward's split plan, so
    the backward must run that plan whatever the process-wide knobs say by then — the halves
    checks against fp64, and the bits of a run with the forward's values held throughout."""
    N, H, V = SPLIT_SHAPE
    if masked:
        h, w, y, gout, live = _masked_inputs(N, H, V, "some")
        mask, t = live.long(), _truth(N, H, V, mask_kind="some")
    else:
        h, w, y, gout = _case(N, H, V)
        live, mask, t = None, None, _truth(N, H, V)
    got = _autograd(h, w, y, gout, "saved_p", mask=mask, fwd_knobs=fwd_knobs, bwd_knobs=bwd_knobs)
    _check(f"fwd {fwd_knobs} bwd {bwd_knobs} masked={masked}", t, got[3], got[4], got[2], got[0], got[1], live=live)
    held = _autograd(h, w, y, gout, "saved_p", mask=mask, fwd_knobs=fwd_knobs, bwd_knobs=fwd_knobs)
    assert torch.equal(got[3], held[3]) and torch.equal(got[4], held[4])


def test_backward_refuses_what_is_no_plan_token():
    """trlx_lmhead_logprobs_bwd_ex2 checks its plan argument before anything else: a value that
    no forward returned is TRLX_ERR_ARG."""
    for bad in (0, 3, (0x4C50 << 32) | 9, (0x4C50 << 32) | (2 << 8) | (2 << 16)):
        with pytest.raises(ValueError, match=r"status 5"):
            L.call("trlx_lmhead_logprobs_bwd_ex2", None, 0, None, 0, 0, 0, 0, None, 0, None, None, 0, None, None, None,
                   0, 0, None, 0, 0, None, None, bad, None)


# ------------------------------------------------------------------ A2: the mask edited in between
def test_int64_mask_edited_before_backward_is_refused():
    """An int64 mask on the device is the tensor the backward rebuilds the compaction from (no
    copy): it is saved with the node, so an in-place edit raises autograd's error instead of
    pairing the forward's P / records with another token order."""
    N, H, V = SHAPES[0]
    h, w, y, gout, live = _masked_inputs(N, H, V, "some")
    m = live.long()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        _autograd(h, w, y, gout, "saved_p", mask=m, between=m.zero_)


@pytest.mark.parametrize("plan", PLANS)
def test_bool_mask_edited_before_backward_has_no_effect(plan):
    N, H, V = SHAPES[0]
    h, w, y, gout, live = _masked_inputs(N, H, V, "some")
    want = _autograd(h, w, y, gout, plan, mask=live.clone())
    m = live.clone()
    got = _autograd(h, w, y, gout, plan, mask=m, between=m.zero_)
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
    _check(f"bool mask edited {plan}", _truth(N, H, V, mask_kind="some"), got[3], got[4], live=live)


# ------------------------------------------------------------------ A3: a float mask
def _float_mask(N):
    m = torch.tensor([0.0, 0.5, 1.0], device=DEV)[torch.randint(0, 3, (N,), generator=torch.Generator().manual_seed(N)).to(DEV)]
    m[0], m[1], m[2] = 0.0, 0.5, 1.0
    return m


def test_float_mask_is_live_where_nonzero():
    """Weights in {0, 0.5, 1}: 0.5 keeps the token — the grad path, the no-grad path and the
    other-H fallback give the bits of the bool mask `mask != 0`."""
    N, H, V = SHAPES[0]
    h, w, y, gout = _case(N, H, V)
    mf = _float_mask(N)
    mb = mf != 0
    assert int((mf == 0.5).sum()) > 0 and int((mf == 0).sum()) > 0
    got = _autograd(h, w, y, gout, "saved_p", mask=mf)
    want = _autograd(h, w, y, gout, "saved_p", mask=mb)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert (got[0][mf == 0.5] != 0).all()
    with torch.no_grad():
        a = P.lm_head_logprobs(h, w, y, out_dtype=F32, mask=mf)
        b = P.lm_head_logprobs(h, w, y, out_dtype=F32, mask=mb)
    assert torch.equal(a, b) and (a[mf == 0.5] != 0).all()
    # H = 256: hipBLASLt logits + logprobs_from_logits under autograd
    N, H, V = 77, 256, 1031
    h, w, y = (x.to(DEV) for x in _operands(N, H, V, 3))
    gout = torch.randn(N, generator=torch.Generator().manual_seed(1)).to(DEV)
    mf = _float_mask(N)
    outs = []
    for m in (mf, mf != 0):
        hg, wg = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
        lp = P.lm_head_logprobs(hg, wg, y, out_dtype=F32, mask=m)
        (lp * gout).sum().backward()
        outs.append((lp.detach(), hg.grad, wg.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert (outs[0][0][mf == 0.5] != 0).all() and (outs[0][0][mf == 0] == 0).all()
