"""T5's full-sequence attention backward on the GPU (csrc/t5_attention_bwd.hip, trlx_t5_attention_bwd,
trlx_t5_attention_fwd_lse, t5_attention.t5_attention_train) against the float64 gradient oracle of
tests/t5_attention_bwd_checks.py.

Tolerance (measured, not fixed in advance), per gradient g in {dq, dk, dv, dbias}: e_torch =
max|g_eager - g_oracle| of torch's own bf16 autograd through HF's op order on the device, and
    max|g_kernel - g_oracle| <= 2 * e_torch + one bf16 ulp of max|g_oracle|
(tests/test_t5_attention_bwd_cpu.py shows five wrong backwards more than 10x outside it).

Shapes: B 2, nH 3, bf16, d_kv in {64, 128}; lengths 1, around and past every tile edge of the
forward's and the backward's kernels, 200; the encoder under the four masks with NaN in the masked
K / V rows, decoder-causal, cross at (Tq, S) pairs under the masks.  Beside the rule, checks no
tolerance can hide: the forward's bits, exact reproducibility of dq / dk / dv (second run, strided
operands, a batch row alone, with and without dbias), exact zeros, the causal range, the C entry's
canaries and refusals, the memory the autograd node holds, the shared table's weight gradient.

TRLX_T5_ATTENTION_BWD_PARITY_OUT=<file>: the measured figures are written there
(profiles/t5_attention_bwd_parity.json is such a run).
"""
import ctypes
import json
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C
import t5_attention_bwd_checks as CB

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TR = P.t5_attention_train
TILES = [(P.t5_attention.Q_TILE, P.t5_attention.KV_TILE), (TR.DQ_Q_TILE, TR.DQ_KV_TILE), (TR.DKV_Q_TILE, TR.DKV_K_TILE)]
SIZES = CB.sizes(TILES)
CROSS = CB.cross_sizes(TILES)
_FIGURES = {}
print(f"t5_attention_bwd tiles (rows, columns): {TILES}; sizes {SIZES}; cross {CROSS}")


def bits(x):
    return x.detach().contiguous().view(torch.int16).cpu()


def dev(*xs):
    return [None if x is None else x.to(DEV) for x in xs]


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_ATTENTION_BWD_PARITY_OUT")
    if path and _FIGURES:
        cases = [_FIGURES[k] for k in sorted(_FIGURES)]
        with open(path, "w") as f:
            json.dump({"rule": "per gradient: e_kernel <= 2 * e_torch + one bf16 ulp of max|oracle|; e = max abs error "
                               "against the float64 autograd oracle, e_torch = torch's bf16 autograd on the device",
                       "device": torch.cuda.get_device_name(0), "tiles_rows_columns": TILES,
                       "worst_ratio": max(c["ratio"] for c in cases), "cases": cases}, f, indent=1)


def train_call(q, k, v, table, mk, causal, dout, want_dbias=True):
    """out and the gradients of t5_attention_train on device tensors in [B, nH, T, d]."""
    q, k, v = (x.detach().clone().requires_grad_() for x in (q, k, v))
    leaves = [q, k, v]
    if table is not None:
        table = table.detach().clone().requires_grad_(want_dbias)
        if want_dbias:
            leaves.append(table)
    out = TR(q, k, v, bias=table, key_mask=mk, causal=causal)
    g = torch.autograd.grad(out, leaves, dout)
    return dict(out=out.detach(), dq=g[0], dk=g[1], dv=g[2], dbias=g[3] if len(g) > 3 else None)


def run_case(mode, d, Tq, S, kind):
    """One parity case: the kernels on NaN-poisoned masked rows, the eager autograd on zeroed ones."""
    c = C.case(d, Tq, S, kind)
    mask = c["mask"]
    bidir, causal = mode == "encoder", mode == "decoder"
    dout = CB.make_dout(d, Tq, S)
    table64 = None if mode == "cross" else CB.table_from(c["W"], Tq, S, bidir)
    want = CB.oracle_grads(c["q"], c["k"], c["v"], dout, table64, mask, causal)
    q, mk, g = dev(c["q"], mask, dout)
    table = None if table64 is None else P.t5_relative_bias_offsets(c["W"].to(DEV), Tq, S, bidir)
    if table is not None:
        assert torch.equal(table.cpu().double(), table64)
    kp, vp = dev(C.poison(c["k"], mask), C.poison(c["v"], mask))
    got = train_call(q, kp, vp, table, mk, causal, g)
    fwd = P.t5_attention(q, kp, vp, bias=table, key_mask=mk, causal=causal)
    assert torch.equal(bits(got["out"]), bits(fwd))                      # the lse entry's out is the forward's
    for n, ref in (("dq", q), ("dk", kp), ("dv", vp)):
        assert got[n].dtype == torch.bfloat16 and got[n].shape == ref.shape and bool(torch.isfinite(got[n]).all()), n
    if mask is not None:
        gone = (mk == 0)[:, None, :, None]
        assert float(got["dk"].float().masked_select(gone).abs().sum()) == 0.0
        assert float(got["dv"].float().masked_select(gone).abs().sum()) == 0.0
    kz, vz = dev(C.poison(c["k"], mask, 0.0), C.poison(c["v"], mask, 0.0))
    yard = CB.eager_grads(q, kz, vz, g, table, mk, causal)
    figs = CB.judge(got, yard, want)
    for n, (e_k, e_t, lim) in figs.items():
        fig = dict(mode=mode, d_kv=d, Tq=Tq, S=S, mask=kind, grad=n, e_torch=e_t, e_kernel=e_k, bound=lim,
                   ratio=e_k / lim if lim > 0 else (0.0 if e_k == 0 else float("inf")), max_abs=float(want[n].abs().max()))
        _FIGURES[(mode, d, Tq, S, kind, n)] = fig
        print(fig)
    for n, (e_k, e_t, lim) in figs.items():
        assert e_k <= lim, (n, figs)
    assert set(figs) == ({"dq", "dk", "dv"} if table is None else set(CB.GRADS))


def test_tiles_match_the_library():
    t = [ctypes.c_int(0) for _ in range(4)]
    _lib.call("trlx_t5_attention_bwd_tiles", *[ctypes.byref(x) for x in t])
    assert [x.value for x in t] == [TR.DQ_Q_TILE, TR.DQ_KV_TILE, TR.DKV_K_TILE, TR.DKV_Q_TILE]


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("kind", C.MASKS)
@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("d", C.D_KVS)
def test_encoder_parity(d, T, kind):
    run_case("encoder", d, T, T, kind)


@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("d", C.D_KVS)
def test_decoder_causal_parity(d, T):
    run_case("decoder", d, T, T, "none")


@pytest.mark.parametrize("kind", C.MASKS)
@pytest.mark.parametrize("Tq,S", CROSS)
@pytest.mark.parametrize("d", C.D_KVS)
def test_cross_parity(d, Tq, S, kind):
    run_case("cross", d, Tq, S, kind)


# ------------------------------------------------------------------ checks no tolerance can hide
def encoder_setup(d, T, kind="holes"):
    c = C.case(d, T, T, kind)
    q, k, v, mk, W, g = dev(c["q"], c["k"], c["v"], c["mask"], c["W"], CB.make_dout(d, T, T))
    table = P.t5_relative_bias_offsets(W, T, T, True)
    return q, k, v, mk, table, g, train_call(q, k, v, table, mk, False, g)


def same_bits(a, b, names=("dq", "dk", "dv")):
    return all(torch.equal(bits(a[n]), bits(b[n])) for n in names)


@pytest.mark.parametrize("d", C.D_KVS)
def test_dq_dk_dv_are_reproducible_and_do_not_depend_on_strides_or_dbias(d):
    T = 2 * TR.DKV_Q_TILE + 3
    q, k, v, mk, table, g, ref = encoder_setup(d, T)
    assert same_bits(train_call(q, k, v, table, mk, False, g), ref)                     # a second run
    assert same_bits(train_call(q, k, v, table, mk, False, g, want_dbias=False), ref)   # the dbias=None path
    # strided operands: a fused [B, T, 3*nH*d] projection's slices, bthd, HF's bhtd view of bthd
    bthd = [x.transpose(1, 2).contiguous() for x in (q, k, v)]
    qkv = torch.cat([x.flatten(2) for x in bthd], dim=2).requires_grad_()
    inner = C.NH * d
    tb = table.clone().requires_grad_()
    out = TR(*[qkv[:, :, i * inner:(i + 1) * inner] for i in range(3)], bias=tb, key_mask=mk, n_heads=C.NH)
    assert torch.equal(bits(out), bits(ref["out"]))
    gq, gt = torch.autograd.grad(out, [qkv, tb], g)
    assert gq.shape == qkv.shape
    for i, n in enumerate(("dq", "dk", "dv")):
        got = gq[:, :, i * inner:(i + 1) * inner].unflatten(2, (C.NH, d)).transpose(1, 2)
        assert torch.equal(bits(got), bits(ref[n])), n
    leaves = [x.clone().requires_grad_() for x in bthd]
    out = TR(*leaves, bias=table, key_mask=mk, layout="bthd")
    gs = torch.autograd.grad(out, leaves, g)
    for x, n in zip(gs, ("dq", "dk", "dv")):
        assert x.shape == bthd[0].shape and torch.equal(bits(x.transpose(1, 2)), bits(ref[n])), n
    gexp = g[:, :, :1].expand_as(g)                                                     # a dO the kernel cannot read in place
    a = train_call(q, k, v, table, mk, False, gexp)
    assert same_bits(a, train_call(q, k, v, table, mk, False, gexp.contiguous()))


@pytest.mark.parametrize("d", C.D_KVS)
def test_a_batch_row_alone_gives_its_bits_in_the_batch(d):
    T = TR.DKV_K_TILE + 1
    q, k, v, mk, table, g, ref = encoder_setup(d, T, "left")
    alone = train_call(q[1:2], k[1:2], v[1:2], table, mk[1:2], False, g[1:2])
    for n in ("dq", "dk", "dv"):
        assert torch.equal(bits(alone[n][0]), bits(ref[n][1])), n


@pytest.mark.parametrize("d", C.D_KVS)
def test_a_fully_masked_row_gives_exact_zeros(d):
    T = TR.DQ_KV_TILE + 1
    q, k, v, mk, table, g, ref = encoder_setup(d, T, "right")
    mk0 = mk.clone()
    mk0[0] = 0
    got = train_call(q, C.poison(k, mk0), C.poison(v, mk0), table, mk0, False, g)
    for n in ("dq", "dk", "dv"):
        assert float(got[n][0].float().abs().max()) == 0.0 and bool(torch.isfinite(got[n]).all()), n
        assert torch.equal(bits(got[n][1]), bits(ref[n][1])), n
    assert bool(torch.isfinite(got["dbias"]).all())


@pytest.mark.parametrize("d", C.D_KVS)
def test_a_causal_call_takes_nothing_from_the_queries_below_a_key_block(d):
    """dK / dV of the keys from DKV_K_TILE on keep their bits when the q and dO rows below DKV_K_TILE
    hold NaN (those query tiles are not loaded for that block of keys), and so do the dQ rows from
    DKV_K_TILE on: the rows the forward's causal-range test treats as unread, mirrored."""
    T, E = 200, TR.DKV_K_TILE
    c = C.case(d, T, T)
    q, k, v, W, g = dev(c["q"], c["k"], c["v"], c["W"], CB.make_dout(d, T, T))
    table = P.t5_relative_bias_offsets(W, T, T, False)
    ref = train_call(q, k, v, table, None, True, g, want_dbias=False)
    q2, g2 = q.clone(), g.clone()
    q2[:, :, :E] = float("nan")
    g2[:, :E] = float("nan")
    got = train_call(q2, k, v, table, None, True, g2, want_dbias=False)
    for n in ("dk", "dv", "dq"):
        assert torch.equal(bits(got[n][:, :, E:]), bits(ref[n][:, :, E:])), n


def c_args(tq, tk, tv, tout, tg, tlse, tdq, tdk, tdv, ws, d, nq, ns, **over):
    """TrlxT5AttentionBwdArgs on [B, nH, T, d] q / k / v, [B, T, nH*d] out / g and given outputs (tensor, strides)."""
    kw = dict(lse=tlse.data_ptr(), bias_by_offset=None, key_mask=None, dbias=None, workspace=ws.data_ptr(),
              workspace_bytes=ws.numel(), B=C.B, n_heads=C.NH, d_kv=d, Tq=nq, S=ns, dtype=_lib.BF16, causal=0)
    for f, p, x in (("q", "q", tq), ("k", "k", tk), ("v", "v", tv)):
        kw[f], kw[f"{p}_stride_b"], kw[f"{p}_stride_t"], kw[f"{p}_stride_h"] = x.data_ptr(), x.stride(0), x.stride(2), x.stride(1)
    for f, p, x in (("out", "o", tout), ("dout", "do", tg)):
        kw[f], kw[f"{p}_stride_b"], kw[f"{p}_stride_t"], kw[f"{p}_stride_h"] = x.data_ptr(), x.stride(0), x.stride(1), d
    for p, (x, sb, st) in (("dq", tdq), ("dk", tdk), ("dv", tdv)):
        kw[p], kw[f"{p}_stride_b"], kw[f"{p}_stride_t"], kw[f"{p}_stride_h"] = x.data_ptr(), sb, st, d
    kw.update(over)
    return _lib.T5AttentionBwdArgs(**kw)


@pytest.mark.parametrize("T", [1, TR.DQ_KV_TILE + 1, TR.DKV_K_TILE + 1])
@pytest.mark.parametrize("d", C.D_KVS)
def test_c_entry_writes_a_fused_buffer_and_keeps_the_canaries(d, T):
    """dq / dk / dv into the three slices of one [B, T, 3*nH*d + gaps] buffer; lse and dbias inside larger
    buffers: every element around and between them keeps its fill."""
    c = C.case(d, T, T, "holes")
    q, k, v, mk, W, g = dev(c["q"], c["k"], c["v"], c["mask"], c["W"], CB.make_dout(d, T, T))
    table = P.t5_relative_bias_offsets(W, T, T, True)
    ref = train_call(q, k, v, table, mk, False, g)
    inner, gap, pad = C.NH * d, 8, 16
    row = 3 * (inner + gap) + gap
    # forward with lse between canary rows
    out = torch.empty(C.B, T, inner, dtype=torch.bfloat16, device=DEV)
    lse_buf = torch.full((C.B * C.NH * T + 2 * pad,), 7.0, device=DEV)
    lse = lse_buf[pad:pad + C.B * C.NH * T]
    fa = _lib.T5AttentionArgs(
        q=q.data_ptr(), q_stride_b=q.stride(0), q_stride_t=q.stride(2), q_stride_h=q.stride(1),
        k=k.data_ptr(), k_stride_b=k.stride(0), k_stride_t=k.stride(2), k_stride_h=k.stride(1),
        v=v.data_ptr(), v_stride_b=v.stride(0), v_stride_t=v.stride(2), v_stride_h=v.stride(1),
        out=out.data_ptr(), o_stride_b=T * inner, o_stride_t=inner, o_stride_h=d, bias_by_offset=table.data_ptr(),
        key_mask=mk.data_ptr(), B=C.B, n_heads=C.NH, d_kv=d, Tq=T, S=T, dtype=_lib.BF16, causal=0)
    _lib.call("trlx_t5_attention_fwd_lse", ctypes.byref(fa), lse.data_ptr(), _lib.stream_of(out))
    assert torch.equal(bits(out), bits(ref["out"]))
    buf = torch.full((C.B * T + 2, row), 7.0, dtype=torch.bfloat16, device=DEV)
    body = buf[1:1 + C.B * T]
    outs = [(body[:, gap + i * (inner + gap):], T * row, row) for i in range(3)]
    db_buf = torch.full((C.NH * (2 * T - 1) + 2 * pad,), 7.0, device=DEV)
    db = db_buf[pad:pad + C.NH * (2 * T - 1)]
    ws = torch.empty(_lib.query("trlx_t5_attention_bwd_workspace_bytes", C.B, C.NH, T), dtype=torch.uint8, device=DEV)
    a = c_args(q, k, v, out, g, lse, *outs, ws, d, T, T, bias_by_offset=table.data_ptr(), key_mask=mk.data_ptr(),
               dbias=db.data_ptr())
    _lib.call("trlx_t5_attention_bwd", ctypes.byref(a), _lib.stream_of(out))
    torch.cuda.synchronize()
    assert bool((lse_buf[:pad] == 7.0).all()) and bool((lse_buf[pad + lse.numel():] == 7.0).all())
    assert bool((db_buf[:pad] == 7.0).all()) and bool((db_buf[pad + db.numel():] == 7.0).all())
    assert bool((buf[0] == 7.0).all()) and bool((buf[-1] == 7.0).all())
    keep = torch.ones(row, dtype=torch.bool, device=DEV)
    for i, n in enumerate(("dq", "dk", "dv")):
        lo = gap + i * (inner + gap)
        keep[lo:lo + inner] = False
        got = body[:, lo:lo + inner].reshape(C.B, T, C.NH, d).transpose(1, 2)
        assert torch.equal(bits(got), bits(ref[n])), n
    assert bool((body[:, keep] == 7.0).all())
    # two runs of the same fp32 atomic sum differ by its order only: far inside one bf16 ulp of the largest entry
    want_db = ref["dbias"].double().cpu()
    assert C.max_err(db.reshape(C.NH, 2 * T - 1), want_db) <= C.bf16_ulp(float(want_db.abs().max()))


def test_a_refused_c_call_leaves_the_outputs_untouched():
    d, T = 64, 9
    c = C.case(d, T, T)
    q, k, v, g = dev(c["q"], c["k"], c["v"], CB.make_dout(d, T, T))
    inner = C.NH * d
    out = P.t5_attention(q, k, v)
    lse = torch.zeros(C.B, C.NH, T, device=DEV)
    dq, dk, dv = (torch.full((C.B, T, inner), 7.0, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    db = torch.full((C.NH, 2 * T - 1), 7.0, device=DEV)
    ws = torch.empty(_lib.query("trlx_t5_attention_bwd_workspace_bytes", C.B, C.NH, T), dtype=torch.uint8, device=DEV)
    dense = [(x, T * inner, inner) for x in (dq, dk, dv)]
    for over in (dict(dtype=_lib.F32), dict(d_kv=96), dict(q_stride_t=d + 4), dict(q=q.data_ptr() + 2),
                 dict(causal=1, S=T - 1), dict(Tq=1 << 31), dict(dq_stride_t=d), dict(dk_stride_b=inner),
                 dict(dout=None), dict(lse=None), dict(dq=None), dict(dk=None), dict(dv=None), dict(dv=dk.data_ptr()),
                 dict(dk=dq.data_ptr() + 16), dict(dk=dq.data_ptr() + 2 * (inner - d)),      # dk = dq + 8, + (nH - 1) d elements
                 dict(dq=g.data_ptr()), dict(dv=out.data_ptr()),                              # an output on a read operand
                 dict(dq=q.data_ptr(), dq_stride_b=q.stride(0), dq_stride_t=q.stride(2), dq_stride_h=q.stride(1)),
                 dict(dk=dq.data_ptr() + 32, dk_stride_b=2 * T * inner, dk_stride_t=2 * inner),   # interleaved, other strides
                 dict(do_stride_t=inner + 4), dict(workspace=None), dict(workspace_bytes=8)):
        a = c_args(q, k, v, out, g, lse, *dense, ws, d, T, T, dbias=db.data_ptr(), **over)
        with pytest.raises(ValueError, match="status 5"):
            _lib.call("trlx_t5_attention_bwd", ctypes.byref(a), _lib.stream_of(out))
    fa = _lib.T5AttentionArgs(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), out=dq.data_ptr(), B=C.B, n_heads=C.NH,
                              d_kv=d, Tq=T, S=T, dtype=_lib.BF16, causal=0, o_stride_b=T * inner, o_stride_t=inner,
                              o_stride_h=d, **{f"{n}_stride_{s}": x.stride(i) for n, x in (("q", q), ("k", k), ("v", v))
                                               for s, i in (("b", 0), ("t", 2), ("h", 1))})
    with pytest.raises(ValueError, match="status 5"):
        _lib.call("trlx_t5_attention_fwd_lse", ctypes.byref(fa), None, _lib.stream_of(out))
    torch.cuda.synchronize()
    for x in (dq, dk, dv, db):
        assert bool((x == 7.0).all())
    assert _lib.query("trlx_t5_attention_bwd_workspace_bytes", 0, 1, 1) == -1


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", C.D_KVS)
def test_c_entry_dbias_without_a_bias_table(d, causal):
    """dbias given, bias_by_offset NULL (the bias is 0): dq / dk / dv are the bits of a call with a table of
    zeros, dbias that call's within the order of its atomics."""
    T = TR.DQ_KV_TILE + 1
    c = C.case(d, T, T, "none")
    q, k, v, g = dev(c["q"], c["k"], c["v"], CB.make_dout(d, T, T))
    zeros = torch.zeros(C.NH, 2 * T - 1, device=DEV)
    ref = train_call(q, k, v, zeros, None, causal, g)
    assert float(ref["dbias"].abs().max()) > 0
    inner = C.NH * d
    out, lse = P.t5_attention(q, k, v, causal=causal), torch.empty(C.B, C.NH, T, device=DEV)
    fa = _lib.T5AttentionArgs(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), out=out.data_ptr(), B=C.B, n_heads=C.NH,
                              d_kv=d, Tq=T, S=T, dtype=_lib.BF16, causal=int(causal), o_stride_b=T * inner,
                              o_stride_t=inner, o_stride_h=d,
                              **{f"{n}_stride_{s}": x.stride(i) for n, x in (("q", q), ("k", k), ("v", v))
                                 for s, i in (("b", 0), ("t", 2), ("h", 1))})
    _lib.call("trlx_t5_attention_fwd_lse", ctypes.byref(fa), lse.data_ptr(), _lib.stream_of(out))
    assert torch.equal(bits(out), bits(ref["out"]))
    dq, dk, dv = (torch.empty(C.B, T, inner, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    db = torch.full((C.NH, 2 * T - 1), 7.0, device=DEV)
    ws = torch.empty(_lib.query("trlx_t5_attention_bwd_workspace_bytes", C.B, C.NH, T), dtype=torch.uint8, device=DEV)
    a = c_args(q, k, v, out, g, lse, *[(x, T * inner, inner) for x in (dq, dk, dv)], ws, d, T, T, dbias=db.data_ptr(),
               causal=int(causal))
    _lib.call("trlx_t5_attention_bwd", ctypes.byref(a), _lib.stream_of(out))
    torch.cuda.synchronize()
    for x, n in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
        assert torch.equal(bits(x.reshape(C.B, T, C.NH, d).transpose(1, 2)), bits(ref[n])), n
    want_db = ref["dbias"].double().cpu()
    assert C.max_err(db, want_db) <= C.bf16_ulp(float(want_db.abs().max()))


def test_the_autograd_node_holds_nothing_of_size_tq_x_s():
    Bm, nH, T, d = 1, 2, 1024, 64
    g0 = torch.Generator().manual_seed(5)
    q, k, v = ((torch.randn(Bm, nH, T, d, generator=g0) * d ** -0.25).to(torch.bfloat16).to(DEV).requires_grad_()
               for _ in range(3))
    W = torch.randn(C.NUM_BUCKETS, nH, generator=g0).to(DEV).requires_grad_()
    buckets = P.t5_relative_bias_buckets(T, T, True, device=DEV)
    dout = torch.randn(Bm, T, nH * d, generator=g0).to(torch.bfloat16).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    table = W.float()[buckets].t().contiguous()
    out = TR(q, k, v, bias=table, key_mask=None)
    out.backward(dout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise over forward + backward: {rise} bytes; one bf16 score tensor: {Bm * nH * T * T * 2}")
    assert all(x.grad is not None for x in (q, k, v, W))
    assert rise < Bm * nH * T * T * 2


@pytest.mark.parametrize("d", C.D_KVS)
def test_two_layers_share_one_table_and_the_weight_gets_both_gradients(d):
    T = TR.DQ_KV_TILE + 1
    cs = [C.case(d, T, T, "right", seed=s) for s in (0, 1)]
    mask = cs[0]["mask"]
    W = cs[0]["W"]
    douts = [CB.make_dout(d, T, T, seed=s) for s in (0, 1)]
    idx = CB.bucket_index(T, T, True)
    # oracle: float64, the two layers' table gradients scattered to the weight
    want = torch.zeros(C.NUM_BUCKETS, C.NH, dtype=torch.float64)
    yard = torch.zeros(C.NUM_BUCKETS, C.NH, dtype=torch.float64)
    for c, g in zip(cs, douts):
        w = CB.oracle_grads(c["q"], c["k"], c["v"], g, CB.table_from(W, T, T, True), mask, False)
        want.index_add_(0, idx, w["dbias"].t())
        q, k, v, mk, gd = dev(c["q"], c["k"], c["v"], mask, g)
        y = CB.eager_grads(q, k, v, gd, P.t5_relative_bias_offsets(W.to(DEV), T, T, True), mk, False)
        yard.index_add_(0, idx, y["dbias"].double().cpu().t())
    Wd = W.to(DEV).requires_grad_()
    buckets = P.t5_relative_bias_buckets(T, T, True, device=DEV)
    assert torch.equal(buckets.cpu(), idx)
    table = Wd.float()[buckets].t().contiguous()
    loss = 0
    for c, g in zip(cs, douts):
        q, mk, gd = dev(c["q"], mask, g)
        kp, vp = dev(C.poison(c["k"], mask), C.poison(c["v"], mask))
        loss = loss + (TR(q, kp, vp, bias=table, key_mask=mk).float() * gd.float()).sum()
    loss.backward()
    e_k, e_t = C.max_err(Wd.grad, want), C.max_err(yard, want)
    print(dict(d_kv=d, e_kernel=e_k, e_torch=e_t, bound=C.bound(e_t, want)))
    assert e_k <= C.bound(e_t, want)
