"""Host-side checks of T5's full-sequence attention backward (no GPU): t5_attention_train's float64
fallback against the gradient oracle, t5_relative_bias_buckets against the oracle's Python buckets
and the offset table, the weight gradient through the table against HF-style compute_bias, that the
GPU test's rule tells five wrong backwards from a right one, the argument errors, and the header /
binding checks that need no device."""
import ctypes
import os
import subprocess

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C
import t5_attention_bwd_checks as CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TR = P.t5_attention_train
MODES = {"encoder": (True, False, "holes", 5, 7), "decoder": (False, True, "none", 7, 7), "cross": (None, False, "holes", 5, 7)}


# ------------------------------------------------------------------ the float64 fallback
@pytest.mark.parametrize("mode", list(MODES))
def test_train_on_cpu_float64_matches_the_oracle(mode):
    bidir, causal, kind, Tq, S = MODES[mode]
    if mode == "encoder":
        S = Tq = 7
    c = C.case(64, Tq, S, kind)
    dout = CB.make_dout(64, Tq, S)
    table = None if bidir is None else CB.table_from(c["W"], Tq, S, bidir)
    want = CB.oracle_grads(c["q"], c["k"], c["v"], dout, table, c["mask"], causal)
    q, k, v = (c[n].double().requires_grad_() for n in "qkv")
    leaves = [q, k, v]
    if table is not None:
        table = table.clone().requires_grad_()
        leaves.append(table)
    out = TR(q, k, v, bias=table, key_mask=c["mask"], causal=causal)
    assert out.dtype == torch.float64
    grads = torch.autograd.grad(out, leaves, dout.double())
    got = dict(zip(("dq", "dk", "dv", "dbias"), grads), out=out.detach())
    for n in ("out",) + CB.GRADS:
        if want.get(n) is None:
            continue
        assert got[n].shape == want[n].shape
        assert C.max_err(got[n], want[n]) <= 1e-9 * float(want[n].abs().max()), n


def test_train_without_grad_is_t5_attention():
    c = C.case(64, 5, 7, "right", dtype=torch.float32)
    table = P.t5_relative_bias_offsets(c["W"], 5, 7, True)
    want = P.t5_attention(c["q"], c["k"], c["v"], bias=table, key_mask=c["mask"])
    assert torch.equal(TR(c["q"], c["k"], c["v"], bias=table, key_mask=c["mask"]), want)
    qg = c["q"].clone().requires_grad_()
    with torch.no_grad():
        assert torch.equal(TR(qg, c["k"], c["v"], bias=table, key_mask=c["mask"]), want)
    out = TR(qg, c["k"], c["v"], bias=table, key_mask=c["mask"])            # fp32: the fallback, differentiable
    assert torch.equal(out.detach(), want)
    (gq,) = torch.autograd.grad(out, [qg], torch.ones_like(out))
    assert gq.shape == qg.shape and bool(torch.isfinite(gq).all())
    gl = c["q"].transpose(1, 2).contiguous().requires_grad_()                # gradients take the given layout
    out = TR(gl, c["k"].transpose(1, 2), c["v"].transpose(1, 2), bias=table, key_mask=c["mask"], layout="bthd")
    assert torch.equal(out.detach(), want)
    assert torch.autograd.grad(out, [gl], torch.ones_like(out))[0].shape == gl.shape


def test_train_without_grad_is_t5_attention_in_float64_too():
    """float64 with gradients keeps its softmax in float64; without, the call is t5_attention and
    returns its bits (an fp32 softmax), under no_grad as well."""
    c = C.case(64, 5, 7, "right", dtype=torch.float64)
    table = P.t5_relative_bias_offsets(c["W"], 5, 7, True)
    want = P.t5_attention(c["q"], c["k"], c["v"], bias=table, key_mask=c["mask"])
    assert torch.equal(TR(c["q"], c["k"], c["v"], bias=table, key_mask=c["mask"]), want)
    assert torch.equal(TR(c["q"], c["k"], c["v"], bias=table.double(), key_mask=c["mask"]), want)
    qg = c["q"].clone().requires_grad_()
    with torch.no_grad():
        assert torch.equal(TR(qg, c["k"], c["v"], bias=table, key_mask=c["mask"]), want)
    exact = TR(qg, c["k"], c["v"], bias=table, key_mask=c["mask"])
    assert exact.requires_grad and C.max_err(exact, want.double()) < 1e-5      # the fp32 softmax's distance, no more


def test_t5_attention_itself_still_raises_with_a_grad_operand():
    c = C.case(64, 5, 7, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="forward only"):
        P.t5_attention(c["q"].clone().requires_grad_(), c["k"], c["v"])


# ------------------------------------------------------------------ buckets, table, weight gradient
@pytest.mark.parametrize("bidirectional", [True, False])
@pytest.mark.parametrize("Tq", [1, 7, 200])
@pytest.mark.parametrize("S", [1, 7, 200])
def test_buckets_equal_the_oracle_buckets_and_the_table(bidirectional, Tq, S):
    b = P.t5_relative_bias_buckets(Tq, S, bidirectional)
    assert b.dtype == torch.int64 and tuple(b.shape) == (Tq + S - 1,)
    assert b.tolist() == [C.bucket(o, bidirectional) for o in range(-(Tq - 1), S)]
    W = torch.randn(C.NUM_BUCKETS, 3, generator=torch.Generator().manual_seed(1))
    assert torch.equal(W.float()[b].t(), P.t5_relative_bias_offsets(W, Tq, S, bidirectional))


@pytest.mark.parametrize("bidirectional,causal", [(True, False), (False, True)])
def test_the_weight_gradient_through_the_table_is_compute_bias_autograd(bidirectional, causal):
    """HF-style compute_bias: weight[bucket(j - i)] as a [nH, Tq, S] tensor added to the scores."""
    T = 9
    c = C.case(64, T, T, "none")
    dout = CB.make_dout(64, T, T).double()
    q, k, v = (c[n].double() for n in "qkv")
    W1 = c["W"].double().requires_grad_()
    table = W1[P.t5_relative_bias_buckets(T, T, bidirectional)].t().contiguous()
    out = TR(q, k, v, bias=table, causal=causal)
    (g1,) = torch.autograd.grad(out, [W1], dout)
    W2 = c["W"].double().requires_grad_()
    want = C.oracle(q, k, v, W2, bidirectional, causal=causal)       # C.oracle_bias is compute_bias in float64
    (g2,) = torch.autograd.grad(want, [W2], dout)
    assert C.max_err(out, want.detach()) <= 1e-9 * float(want.abs().max())
    assert C.max_err(g1, g2.detach()) <= 1e-9 * float(g2.abs().max())


# ------------------------------------------------------------------ the rule tells wrong backwards apart
def _round(grads):
    return {n: (None if x is None else x.to(torch.bfloat16)) for n, x in grads.items()}


WRONG = {
    "delta_dropped": (dict(drop_delta=True), "encoder", ("dq", "dk", "dbias")),
    "bias_one_offset_off": (dict(bias_shift=1), "encoder", ("dq", "dk", "dv", "dbias")),
    "live_key_dropped": (dict(drop_key="live"), "encoder", ("dq", "dk", "dv", "dbias")),
    "causal_boundary_one_off": (dict(causal_shift=-1), "decoder", ("dq", "dk", "dv", "dbias")),
    "dbias_without_the_batch_sum": (dict(per_batch_dbias=True), "encoder", ("dbias",)),
}


@pytest.mark.parametrize("T", [65, 200])
@pytest.mark.parametrize("name", list(WRONG))
def test_the_rule_tells_a_wrong_backward_apart(name, T):
    """Each wrong backward, built in float64 and rounded to bf16 as a kernel's result would be, lands
    more than 10x outside the bound in at least the gradients it must disturb; the right one, rounded
    the same way, lands inside."""
    kw, mode, hit = WRONG[name]
    d = 64
    bidir, causal = mode == "encoder", mode == "decoder"
    kind = "right" if mode == "encoder" else "none"
    c = C.case(d, T, T, kind)
    mask = c["mask"]
    dout = CB.make_dout(d, T, T)
    table = CB.table_from(c["W"], T, T, bidir)
    want = CB.oracle_grads(c["q"], c["k"], c["v"], dout, table, mask, causal)
    kz, vz = C.poison(c["k"], mask, 0.0), C.poison(c["v"], mask, 0.0)
    yard = CB.eager_grads(c["q"], kz, vz, dout, table.float(), mask, causal)     # CPU bf16 autograd as e_torch
    right = CB.judge(_round(want), yard, want)
    for n, (e_k, e_t, lim) in right.items():
        assert e_k <= lim, (n, right)
    kw = dict(kw)
    if kw.get("drop_key") == "live":
        b0 = 1
        kw["drop_key"] = (b0, int(torch.nonzero(mask[b0])[0]))
    wrong = CB.oracle_grads(c["q"], c["k"], c["v"], dout, table, mask, causal, **kw)
    figs = CB.judge(_round(wrong), yard, want)
    print(name, T, {n: (e_k / lim) for n, (e_k, e_t, lim) in figs.items()})
    for n in hit:
        e_k, e_t, lim = figs[n]
        assert e_k > 10 * lim, (name, n, figs[n])


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    q = torch.zeros(2, 3, 5, 64, dtype=torch.float64, requires_grad=True)
    k = torch.zeros(2, 3, 7, 64, dtype=torch.float64)
    with pytest.raises(ValueError, match="causal needs"):
        TR(q, k, k, causal=True)
    with pytest.raises(ValueError, match="disagree"):
        TR(q, k, k[:, :2])
    with pytest.raises(ValueError, match="bias must be"):
        TR(q, k, k, bias=torch.zeros(3, 5 + 7, dtype=torch.float64))
    with pytest.raises(ValueError, match="bias must be"):
        TR(q.float(), k.float(), k.float(), bias=torch.zeros(3, 5 + 7 - 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="key_mask must be"):
        TR(q, k, k, key_mask=torch.ones(2, 6, dtype=torch.int64))
    with pytest.raises(ValueError, match="n_heads"):
        TR(q.flatten(2), k, k)
    with pytest.raises(ValueError, match="layout"):
        TR(q, k, k, layout="hbtd")
    with pytest.raises(ValueError):
        P.t5_relative_bias_buckets(0, 3, True)


# ------------------------------------------------------------------ header, binding, tiles
def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    assert "int trlx_t5_attention_fwd_lse(const TrlxT5AttentionArgs* a, float* lse, void* stream);" in txt
    assert "int trlx_t5_attention_bwd(const TrlxT5AttentionBwdArgs* a, void* stream);" in txt
    res, args = _lib.SIGNATURES["trlx_t5_attention_bwd"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.T5AttentionBwdArgs), ctypes.c_void_p]


def test_struct_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in _lib.T5AttentionBwdArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(TrlxT5AttentionBwdArgs, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(TrlxT5AttentionBwdArgs));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(_lib.T5AttentionBwdArgs, f).offset for f in fields] + [ctypes.sizeof(_lib.T5AttentionBwdArgs)]


def test_tiles_and_workspace_need_no_device():
    t = [ctypes.c_int(0) for _ in range(4)]
    _lib.call("trlx_t5_attention_bwd_tiles", *[ctypes.byref(x) for x in t])
    assert [x.value for x in t] == [TR.DQ_Q_TILE, TR.DQ_KV_TILE, TR.DKV_K_TILE, TR.DKV_Q_TILE]
    assert _lib.query("trlx_t5_attention_bwd_workspace_bytes", 2, 3, 5) >= 4 * 2 * 3 * 5
    assert _lib.query("trlx_t5_attention_bwd_workspace_bytes", 2, 3, 0) == -1
    # the workspace does not grow with S: it is not an argument
    assert len(_lib.SIGNATURES["trlx_t5_attention_bwd_workspace_bytes"][1]) == 3
