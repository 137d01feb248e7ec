"""The ordered bias gradient of T5's attention backward on the GPU (t5_attention_train(bias_grad="ordered"),
trlx_t5_attention_bwd_ordered) at d_kv 64, 128, 256, B 2, nH 3: the backward's own rule against the float64 oracle
at T 1, 33, 129 (two query blocks) and 259 (three, the ring has wrapped), then exact checks of bits, zeros and refusals.
TRLX_T5_ATTENTION_DBIAS_ORDERED_PARITY_OUT=<file> writes the figures (profiles/t5_attention_dbias_ordered_parity.json).
"""
import ctypes
import importlib
import json
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C
import t5_attention_bwd_checks as CB
from test_gpu_t5_attention_bwd import bits, dev, c_args

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D_KVS = (64, 128, 256)
SIZES = (1, 33, 129, 259)
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_ATTENTION_DBIAS_ORDERED_PARITY_OUT")
    if path and _FIGURES:
        cases = [_FIGURES[k] for k in sorted(_FIGURES)]
        with open(path, "w") as f:
            json.dump({"rule": "per gradient: e_kernel <= 2 * e_torch + one bf16 ulp of max|oracle|",
                       "device": torch.cuda.get_device_name(0), "worst_ratio": max(c["ratio"] for c in cases),
                       "cases": cases}, f, indent=1)


same = lambda x, y: torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))  # noqa: E731


def train(q, k, v, table, mk, causal, dout, bias_grad="ordered", layout="bhtd"):
    """out and the gradients of t5_attention_train on device tensors; q, k, v in `layout`."""
    leaves = [x.detach().clone().requires_grad_() for x in (q, k, v, table)]
    out = P.t5_attention_train(*leaves[:3], bias=leaves[3], key_mask=mk, causal=causal, layout=layout, bias_grad=bias_grad)
    return dict(zip(("out", "dq", "dk", "dv", "dbias"), (out.detach(), *torch.autograd.grad(out, leaves, dout))))


def setup(d, T, kind="holes", causal=False):
    c = C.case(d, T, T, kind)
    q, k, v, mk, W, g = dev(c["q"], c["k"], c["v"], c["mask"], c["W"], CB.make_dout(d, T, T))
    return q, k, v, mk, P.t5_relative_bias_offsets(W, T, T, not causal), g


@pytest.mark.parametrize("mode,kind", [("encoder", "none"), ("encoder", "holes"), ("encoder", "left"), ("decoder", "none")])
@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("d", D_KVS)
def test_parity(d, T, mode, kind):
    c = C.case(d, T, T, kind)
    mask, causal = c["mask"], mode == "decoder"
    dout = CB.make_dout(d, T, T)
    want = CB.oracle_grads(c["q"], c["k"], c["v"], dout, CB.table_from(c["W"], T, T, not causal), mask, causal)
    q, mk, g = dev(c["q"], mask, dout)
    table = P.t5_relative_bias_offsets(c["W"].to(DEV), T, T, not causal)
    got = train(q, *dev(C.poison(c["k"], mask), C.poison(c["v"], mask)), table, mk, causal, g)
    yard = CB.eager_grads(q, *dev(C.poison(c["k"], mask, 0.0), C.poison(c["v"], mask, 0.0)), g, table, mk, causal)
    figs = CB.judge(got, yard, want)
    for n, (e_k, e_t, lim) in figs.items():
        fig = dict(mode=mode, d_kv=d, T=T, mask=kind, grad=n, e_torch=e_t, e_kernel=e_k, bound=lim,
                   ratio=e_k / lim if lim > 0 else (0.0 if e_k == 0 else float("inf")), max_abs=float(want[n].abs().max()))
        _FIGURES[(mode, d, T, kind, n)] = fig
        print(fig)
    assert set(figs) == set(CB.GRADS)
    for n, (e_k, e_t, lim) in figs.items():
        assert e_k <= lim, (n, figs)


@pytest.mark.parametrize("d", D_KVS)
def test_dq_dk_dv_and_out_are_the_default_routes_bits(d):
    q, k, v, mk, table, g = setup(d, 259)
    got, ref = train(q, k, v, table, mk, False, g), train(q, k, v, table, mk, False, g, bias_grad="atomic")
    for n in ("out", "dq", "dk", "dv"):
        assert torch.equal(bits(got[n]), bits(ref[n])), n


@pytest.mark.parametrize("d", D_KVS)
def test_dbias_bits_are_fixed_over_runs_layouts_and_stale_buffers(d):
    T, inner = 259, C.NH * d
    q, k, v, mk, table, g = setup(d, T)
    ref = train(q, k, v, table, mk, False, g)
    assert same(train(q, k, v, table, mk, False, g)["dbias"], ref["dbias"])                       # a second run
    bthd = [x.transpose(1, 2).contiguous() for x in (q, k, v)]
    assert same(train(*bthd, table, mk, False, g, layout="bthd")["dbias"], ref["dbias"])
    qkv = torch.cat([x.flatten(2) for x in bthd], dim=2)                                                 # a fused projection's slices
    tb = table.clone().requires_grad_()
    out = P.t5_attention_train(*[qkv[:, :, i * inner:(i + 1) * inner] for i in range(3)], bias=tb, key_mask=mk,
                               n_heads=C.NH, bias_grad="ordered")
    assert same(torch.autograd.grad(out, [tb], g)[0], ref["dbias"])
    # the C entry on a dbias and a dbias workspace of 0xFF bytes: neither is read before it is written
    M = importlib.import_module("trlx_t5_amd.t5_attention")
    out, lse = M._kernel_forward(*[x.transpose(1, 2) for x in (q, k, v)], table, mk, False, True)
    outs = [(torch.empty(C.B, T, inner, dtype=torch.bfloat16, device=DEV), T * inner, inner) for _ in range(3)]
    ws = torch.empty(_lib.query("trlx_t5_attention_bwd_workspace_bytes", C.B, C.NH, T), dtype=torch.uint8, device=DEV)
    pw = torch.full((_lib.query("trlx_t5_attention_bwd_dbias_workspace_bytes", C.B, C.NH, d, T, T),), 0xFF,
                    dtype=torch.uint8, device=DEV)
    dbias = torch.full((C.NH * (2 * T - 1) * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).view(C.NH, -1)
    a = c_args(q, k, v, out, g, lse, *outs, ws, d, T, T, bias_by_offset=table.data_ptr(), key_mask=mk.data_ptr(),
               dbias=dbias.data_ptr())
    _lib.call("trlx_t5_attention_bwd_ordered", ctypes.byref(a), pw.data_ptr(), pw.numel(), _lib.stream_of(out))
    assert same(dbias, ref["dbias"])


@pytest.mark.parametrize("d", D_KVS)
def test_dead_rows_add_exact_zeros(d):
    q, k, v, mk, table, g = setup(d, 129)
    mk[1] = 0                                                    # batch row 1: no live key, NaN in all of its K / V
    two = train(q, C.poison(k, mk), C.poison(v, mk), table, mk, False, g)["dbias"]
    one = train(q[:1], k[:1], v[:1], table, mk[:1], False, g[:1])["dbias"]
    assert same(two, one) and bool(one.abs().max() > 0)
    q, k, v, _, table, g = setup(d, 129, "none", causal=True)
    causal = train(q, k, v, table, None, True, g)["dbias"]
    assert bool((causal[:, 129:].contiguous().view(torch.int32) == 0).all()) and bool(causal[:, :129].abs().max() > 0)   # j > i


@pytest.mark.parametrize("d", D_KVS)
def test_refusals_leave_the_outputs_alone(d):
    T, inner = 9, C.NH * d
    q, k, v, mk, table, g = setup(d, T)
    out, lse = P.t5_attention(q, k, v), torch.zeros(C.B, C.NH, T, device=DEV)
    outs = [(torch.full((C.B, T, inner), 7.0, dtype=torch.bfloat16, device=DEV), T * inner, inner) for _ in range(3)]
    dbias = torch.full((C.NH, 2 * T - 1), 7.0, device=DEV)
    ws = torch.empty(_lib.query("trlx_t5_attention_bwd_workspace_bytes", C.B, C.NH, T), dtype=torch.uint8, device=DEV)
    need = _lib.query("trlx_t5_attention_bwd_dbias_workspace_bytes", C.B, C.NH, d, T, T)
    assert need == 4 * C.B * C.NH * (T + 127)
    pw = torch.empty(need + 4, dtype=torch.uint8, device=DEV)
    a = c_args(q, k, v, out, g, lse, *outs, ws, d, T, T, bias_by_offset=table.data_ptr(), dbias=dbias.data_ptr())
    for p, n in ((None, need), (pw.data_ptr(), need - 1), (pw.data_ptr() + 2, need)):   # NULL, one byte short, misaligned by 2
        with pytest.raises(ValueError, match="status 5"):
            _lib.call("trlx_t5_attention_bwd_ordered", ctypes.byref(a), p, n, _lib.stream_of(out))
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in (dbias, *[o[0] for o in outs]))
    for bad in ((0, C.NH, d, T, T), (C.B, C.NH, 96, T, T), (C.B, C.NH, d, T, 2 ** 30 + 1)):
        assert _lib.query("trlx_t5_attention_bwd_dbias_workspace_bytes", *bad) == -1
    with pytest.raises(ValueError, match="bias_grad"):
        P.t5_attention_train(q, k, v, bias=table, bias_grad="x")
