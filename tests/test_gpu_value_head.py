"""The fused bf16 value head on the GPU (csrc/value_head.hip k_vhead, trlx_value_head_fwd / _bwd,
value_head.value_head / ValueHead) against the two CPU restatements of tests/value_head_checks.py.

Tolerance (not fixed in advance): for every case e_ref = max|(a) − (b)|, torch's bf16 CPU module
against the fp64 oracle on the same inputs; the kernel must satisfy
    max|kernel − (b)| <= 2·e_ref + 1e-6·max|(b)|
for the values and for each of dh, dW1, db1, dw2, db2 (see value_head_checks).

Shapes: H in {32, 64, 160, 768} (one K step, one MFMA column group, a ragged column slice, the
product size) with N in {1, 65}, and N in {1, 63, 64, 65, 130} (one token, a partial block, an
exact block, one and two over) with H = 64.

TRLX_VALUE_HEAD_PARITY_OUT=<file>: the measured figures of the parity cases are written there
(profiles/value_head_parity.json is such a run).
"""
import json
import os
import sys

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import value_head_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VH = sys.modules["trlx_t5_amd.value_head"]
KEYS = ("h", "w1", "b1", "w2", "b2")
SHAPES = [(1, 32), (65, 32), (1, 64), (63, 64), (64, 64), (65, 64), (130, 64), (1, 160), (65, 160), (1, 768),
          (65, 768)]
_REFS = {}
_FIGURES = {}


def refs(N, H):
    """The case's operands and both restatements, computed once and shared (never modified)."""
    if (N, H) not in _REFS:
        c = C.make_case(N, H, 1000 * H + N)
        args = [c[k] for k in KEYS]
        _REFS[(N, H)] = (c, C.reference_bf16(*args, dv=c["dv"]), C.oracle_fp64(*args, dv=c["dv"]))
    return _REFS[(N, H)]


def dev_ops(c, grad=False):
    return [c[k].to(DEV).requires_grad_(grad) for k in KEYS]


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_VALUE_HEAD_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "max|kernel - fp64 oracle| <= 2 * e_ref + 1e-6 * max|oracle|, "
                               "e_ref = max|torch bf16 CPU - fp64 oracle|",
                       "cases": [_FIGURES[k] for k in sorted(_FIGURES)]}, f, indent=1)


@pytest.mark.parametrize("N,H", SHAPES)
def test_parity_values_and_gradients(N, H):
    c, a, b = refs(N, H)
    ops = dev_ops(c, grad=True)
    v = P.value_head(*ops)
    assert v.dtype == torch.float32 and tuple(v.shape) == (N,)
    v.backward(c["dv"].float().to(DEV))
    torch.cuda.synchronize()
    got = dict(values=v, dh=ops[0].grad, dw1=ops[1].grad, db1=ops[2].grad, dw2=ops[3].grad, db2=ops[4].grad)
    fig = {"N": N, "H": H, "splits": P.value_head_splits(N, H)}
    failed = []
    for k in ("values",) + C.GRADS:
        assert got[k] is not None, k
        if k != "values":   # a gradient has its tensor's dtype and shape
            assert got[k].dtype == torch.bfloat16 and got[k].shape == ops[C.GRADS.index(k)].shape
        e_ref, e_k = C.max_err(a[k], b[k]), C.max_err(got[k], b[k])
        lim = C.bound(e_ref, b[k])
        fig[k] = {"e_ref": e_ref, "e_kernel": e_k, "bound": lim, "max_abs": float(b[k].abs().max())}
        print(f"N={N} H={H} {k}: e_ref={e_ref:.6g} e_kernel={e_k:.6g} bound={lim:.6g}")
        if not e_k <= lim:
            failed.append(k)
    _FIGURES[(H, N)] = fig
    assert not failed, f"over the bound: {failed}: {fig}"


@pytest.mark.parametrize("S", [1, 2, 3, 64])
def test_forced_splits_reproducible_and_stride_independent(S):
    N, H = 65, 160
    c, a, b = refs(N, H)
    ops = dev_ops(c)
    with _lib.tuning(vhead_splits=S):
        s_eff = P.value_head_splits(N, H)
        assert s_eff == (S if S < 64 else 2 * H // 32)   # the cap: one split per 32 columns
        v1 = P.value_head(*ops)
        v2 = P.value_head(*ops)
        # the same rows through a [B, T, H] tensor's last position and behind a one-row offset
        g = torch.Generator().manual_seed(5)
        h3 = torch.randn(N, 3, H, generator=g).to(torch.bfloat16).to(DEV)
        h3[:, -1, :] = ops[0]
        view3 = h3[:, -1, :]
        big = torch.randn(N + 1, H, generator=g).to(torch.bfloat16).to(DEV)
        big[1:] = ops[0]
        view1 = big[1:]
        for view in (view3, view1):   # read in place, not through a copy
            assert not view.is_contiguous() or view.data_ptr() != big.data_ptr()
            assert VH._rows(view, H).data_ptr() == view.data_ptr()
        v3 = P.value_head(view3, *ops[1:])
        v4 = P.value_head(view1, *ops[1:])
        vb = P.value_head(*ops, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert view3.stride(0) == 3 * H and view1.data_ptr() == big.data_ptr() + 2 * H
    for other in (v2, v3, v4):
        assert torch.equal(bits(v1), bits(other))
    assert torch.equal(bits(vb), bits(v1.to(torch.bfloat16)))   # the fp32 result rounded once
    e_ref, e_k = C.max_err(a["values"], b["values"]), C.max_err(v1, b["values"])
    print(f"S={s_eff}: e_ref={e_ref:.6g} e_kernel={e_k:.6g}")
    assert e_k <= C.bound(e_ref, b["values"])
    assert P.value_head_splits(N, H) >= 1   # the knob is restored


def test_splits_are_a_function_of_the_shape():
    ncu = torch.cuda.get_device_properties(DEV).multi_processor_count
    for N, H in [(1, 768), (128, 768), (256, 768), (6144, 768), (12288, 768), (6144, 1024), (65, 32)]:
        want = max(1, min(-(-ncu // -(-N // 64)), 2 * H // 32, 64))
        assert P.value_head_splits(N, H) == want, (N, H)
    assert P.value_head_splits(128, 768) > 1 and 1 <= P.value_head_splits(6144, 768) <= 3
    assert 1 <= P.value_head_splits(12288, 768) <= 3
    assert P.value_head_splits(4, 48) == 0 and P.value_head_splits(0, 64) == 0


@pytest.mark.parametrize("N,H", [(65, 64), (1, 768)])
def test_output_dtype_rounds_once(N, H):
    c, _, _ = refs(N, H)
    ops = dev_ops(c)
    v32 = P.value_head(*ops)
    v16 = P.value_head(*ops, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert v16.dtype == torch.bfloat16 and torch.equal(bits(v16), bits(v32.to(torch.bfloat16)))


def raw_backward(ops, dv, dv_dtype=None):
    """trlx_value_head_bwd itself: (dz, dw2, db1, db2)."""
    h, w1, b1, w2 = ops[:4]
    N, H = h.shape
    dz = torch.full((N, 2 * H), 7.0, dtype=torch.bfloat16, device=DEV)
    dw2 = torch.full((2 * H,), 7.0, dtype=torch.bfloat16, device=DEV)
    db1 = torch.full((2 * H,), 7.0, dtype=torch.bfloat16, device=DEV)
    db2 = torch.full((1,), 7.0, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(_lib.query("trlx_value_head_bwd_workspace_bytes", N, H), dtype=torch.uint8, device=DEV)
    _lib.call("trlx_value_head_bwd", h.data_ptr(), h.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
              dv.data_ptr(), _lib.dtype_code(dv) if dv_dtype is None else dv_dtype, N, H, dz.data_ptr(),
              dw2.data_ptr(), db1.data_ptr(), db2.data_ptr(), _lib.BF16, ws.data_ptr(), _lib.stream_of(h))
    return dz, dw2, db1, db2


@pytest.mark.parametrize("N,H,S", [(65, 64, 0), (65, 160, 3)])
def test_relu_mask_columns_contribute_nothing(N, H, S):
    """Columns whose z is exactly 0 (zero W1 row, b1 = 0) or negative (b1 = -1): nothing forward,
    dz = 0, dw2 = 0, db1 = 0 (torch's relu gradient at 0 is 0)."""
    c = dict(refs(N, H)[0])
    zero_cols = torch.tensor([0, 15, 16, 63, 64, 2 * H - 1])
    neg_cols = torch.tensor([1, 31, 65, 2 * H - 2])
    dead = torch.cat([zero_cols, neg_cols])
    c["w1"] = c["w1"].clone()
    c["b1"] = c["b1"].clone()
    c["w1"][dead] = 0
    c["b1"][zero_cols] = 0
    c["b1"][neg_cols] = -1
    args = [c[k] for k in KEYS]
    a, b = C.reference_bf16(*args, dv=c["dv"]), C.oracle_fp64(*args, dv=c["dv"])
    assert float(b["db1"][dead].abs().max()) == 0 and float(a["dw2"][dead].float().abs().max()) == 0
    with _lib.tuning(vhead_splits=S):
        ops = dev_ops(c, grad=True)
        v = P.value_head(*ops)
        # the dead columns' w2 does not matter: the same bits with it zeroed
        w2z = c["w2"].clone()
        w2z[0, dead] = 0
        vz = P.value_head(ops[0].detach(), ops[1].detach(), ops[2].detach(), w2z.to(DEV), ops[4].detach())
        v.backward(c["dv"].float().to(DEV))
        dz, dw2, db1, db2 = raw_backward([t.detach() for t in ops], c["dv"].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(v), bits(vz))
    e_ref, e_k = C.max_err(a["values"], b["values"]), C.max_err(v, b["values"])
    print(f"mask N={N} H={H}: e_ref={e_ref:.6g} e_kernel={e_k:.6g}")
    assert e_k <= C.bound(e_ref, b["values"])
    dead = dead.to(DEV)
    assert float(dz[:, dead].float().abs().max()) == 0
    assert float(dw2[dead].float().abs().max()) == 0 and float(db1[dead].float().abs().max()) == 0
    assert float(ops[3].grad[0, dead].float().abs().max()) == 0 and float(ops[2].grad[dead].float().abs().max()) == 0
    assert float(ops[1].grad[dead].float().abs().max()) == 0
    # the raw entry and autograd agree, and the live columns are live
    assert torch.equal(bits(dw2), bits(ops[3].grad.reshape(-1))) and torch.equal(bits(db1), bits(ops[2].grad))
    assert torch.equal(bits(db2), bits(ops[4].grad.reshape(-1)))
    live = torch.ones(2 * H, dtype=torch.bool, device=DEV)
    live[dead] = False
    assert float(dz[:, live].float().abs().max()) > 0
    # dz itself: bf16(dv·w2) under the oracle's mask, wherever the oracle's z is not within a
    # rounding of 0 (there the fp32 sum's sign may differ)
    z64 = c["h"].double() @ c["w1"].double().t() + c["b1"].double()
    want = (c["dv"].float()[:, None] * c["w2"].float()).to(torch.bfloat16)
    want = torch.where(z64.float().to(torch.bfloat16) > 0, want, torch.zeros_like(want))
    clear = (z64.abs() > 1e-4) | (z64 == 0)
    assert torch.equal(bits(dz)[clear], bits(want)[clear]) and float(clear.double().mean()) > 0.99


def test_autograd_contract():
    N, H = 65, 64
    c, a, b = refs(N, H)
    ops = dev_ops(c, grad=True)
    dv = c["dv"].float().to(DEV)
    v = P.value_head(*ops)
    assert v.requires_grad and v.grad_fn is not None
    v.backward(dv)
    assert all(t.grad is not None for t in ops)
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        v.backward(dv)
    # an in-place edit of w1 between forward and backward: autograd's version check
    ops = dev_ops(c, grad=True)
    v = P.value_head(*ops)
    with torch.no_grad():
        ops[1].mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        v.backward(dv)
    # no_grad: the same bits, nothing kept
    ops = dev_ops(c, grad=True)
    v_grad = P.value_head(*ops)
    with torch.no_grad():
        v_ng = P.value_head(*ops)
    assert not v_ng.requires_grad and v_ng.grad_fn is None
    assert torch.equal(bits(v_grad), bits(v_ng))
    # bf16 values take a bf16 gradient; retain_graph allows the second backward, same bits
    ops = dev_ops(c, grad=True)
    vb = P.value_head(*ops, out_dtype=torch.bfloat16)
    vb.backward(c["dv"].to(DEV), retain_graph=True)
    g1 = [t.grad.clone() for t in ops]
    for t in ops:
        t.grad = None
    vb.backward(c["dv"].to(DEV))
    torch.cuda.synchronize()
    for x, t in zip(g1, ops):
        assert torch.equal(bits(x), bits(t.grad))
    # only the tensors that ask get a gradient
    ops = dev_ops(c)
    ops[0].requires_grad_(True)
    P.value_head(*ops).backward(dv)
    assert ops[0].grad is not None and all(t.grad is None for t in ops[1:])


def test_module_is_a_drop_in():
    H = 64
    c, a, b = refs(130, H)
    head = P.ValueHead(H).to(DEV)
    head.load_state_dict({"0.weight": c["w1"], "0.bias": c["b1"], "2.weight": c["w2"], "2.bias": c["b2"]}, strict=True)
    h = c["h"].to(DEV).reshape(2, 65, H)
    out = head(h)
    assert tuple(out.shape) == (2, 65, 1) and out.dtype == torch.bfloat16
    assert torch.equal(bits(out), bits(head.values(h, torch.bfloat16)[..., None]))
    assert tuple(head.values(h).shape) == (2, 65) and head.values(h).dtype == torch.float32
    assert out.squeeze(-1).shape == (2, 65)
    e_ref, e_k = C.max_err(a["values"], b["values"]), C.max_err(head.values(h), b["values"])
    assert e_k <= C.bound(e_ref, b["values"])
    # the module trains: every parameter and the input receive a gradient
    h.requires_grad_(True)
    head(h).sum().backward()
    assert h.grad is not None and all(p.grad is not None and p.grad.shape == p.shape for p in head.parameters())
    assert isinstance(P.make_value_head(H, 1), P.ValueHead)


def test_decode_loop_records_the_fused_values():
    """B 4, T 6, V 37, H 64: the decode loop's per-step values land in the recorder as
    v_head.values(h_all) computes them in one go (same inputs, same splits)."""
    B, T, V, H = 4, 6, 37, 64
    g = torch.Generator().manual_seed(11)
    head = P.ValueHead(H).to(DEV)
    h_all = torch.randn(B, T, H, generator=g).to(torch.bfloat16).to(DEV)
    logits = torch.randn(B, T, V, generator=g).to(DEV)
    ref_logits = torch.randn(B, T, V, generator=g).to(DEV)
    rec = P.PPORolloutRecorder(B, T, DEV, pad_token_id=0, eos_token_id=None)
    with _lib.tuning(vhead_splits=2), torch.no_grad():
        for t in range(T):
            values = head.values(h_all[:, t, :])   # a row-strided view, read in place
            P.ppo_sample_step(logits[:, t], ref_logits=ref_logits[:, t], recorder=rec, values=values,
                              u=torch.rand(B, generator=g).to(DEV), cur_len=t)
        want = head.values(h_all)
    torch.cuda.synchronize()
    assert rec.t == T and tuple(want.shape) == (B, T)
    for t in range(T):
        assert torch.equal(bits(rec.values[:, t]), bits(want[:, t])), t


def test_guards_leave_outputs_untouched():
    N, H = 65, 64
    c, _, _ = refs(N, H)
    h, w1, b1, w2, b2 = dev_ops(c)
    out = torch.full((N,), 7.0, device=DEV)
    ws = torch.empty(_lib.query("trlx_value_head_workspace_bytes", N, H), dtype=torch.uint8, device=DEV)
    st = _lib.stream_of(h)

    def fwd(hp=None, ld=H, n=N, hh=H, dt=_lib.F32, w1p=None, b1p=None, wsp=ws.data_ptr(), outp=None):
        _lib.call("trlx_value_head_fwd", h.data_ptr() if hp is None else hp, ld,
                  w1.data_ptr() if w1p is None else w1p, b1.data_ptr() if b1p is None else b1p, w2.data_ptr(),
                  b2.data_ptr(), n, hh, out.data_ptr() if outp is None else outp, dt, wsp, st)

    bad = [dict(hh=48), dict(hh=0), dict(hh=8224), dict(n=0), dict(ld=H - 8), dict(ld=H + 4),
           dict(hp=h.data_ptr() + 2), dict(w1p=w1.data_ptr() + 8), dict(b1p=b1.data_ptr() + 2), dict(dt=_lib.I64),
           dict(dt=7)]
    for kw in bad:
        with pytest.raises(ValueError):
            fwd(**kw)
    with pytest.raises(ValueError):   # NULL h
        _lib.call("trlx_value_head_fwd", None, H, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), N, H,
                  out.data_ptr(), _lib.F32, ws.data_ptr(), st)
    with _lib.tuning(vhead_splits=2):
        with pytest.raises(ValueError):   # splits need the workspace
            fwd(wsp=None)
    with pytest.raises(ValueError):
        _lib.set_tuning("vhead_splits", 65)
    with pytest.raises(ValueError):
        _lib.set_tuning("vhead_splits", -1)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the wrapper's own checks, with device tensors
    for args in ([h.float(), w1, b1, w2, b2], [h, w1[:-1], b1, w2, b2], [h[:, :48], w1, b1, w2, b2],
                 [h, w1, b1, w2, b2.cpu()]):
        with pytest.raises((ValueError, TypeError)):
            P.value_head(*args)
    # backward: sentinels survive a refused call
    dv = c["dv"].to(DEV)
    for kw in (dict(dv_dtype=_lib.I64),):
        with pytest.raises(ValueError):
            raw_backward([h, w1, b1, w2], dv, **kw)
    with pytest.raises(ValueError):
        raw_backward([h[:, :48].contiguous(), w1, b1, w2], dv)
    keep = {}

    def sentinel_backward():
        dz = torch.full((N, 2 * H), 7.0, dtype=torch.bfloat16, device=DEV)
        small = torch.full((2 * H,), 7.0, dtype=torch.bfloat16, device=DEV)
        keep["t"] = (dz, small)
        _lib.call("trlx_value_head_bwd", h.data_ptr(), H, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                  dv.data_ptr(), _lib.BF16, N, H, dz.data_ptr(), small.data_ptr(), small.data_ptr(),
                  small.data_ptr(), _lib.BF16, None, st)   # NULL workspace

    with pytest.raises(ValueError):
        sentinel_backward()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in keep["t"])
    # and the operands are intact: the good call still gives the oracle's values
    fwd()
    torch.cuda.synchronize()
    _, a, b = refs(N, H)
    assert C.max_err(out, b["values"]) <= C.bound(C.max_err(a["values"], b["values"]), b["values"])
