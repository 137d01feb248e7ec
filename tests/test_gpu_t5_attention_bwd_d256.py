"""T5's attention backward at d_kv 256 on the GPU (csrc/t5_attention_bwd_d256.hip behind
trlx_t5_attention_bwd, the lse instantiations of csrc/t5_attention_d256.hip, t5_attention_train): the d 64 / 128
backward's rule and exact checks (tests/test_gpu_t5_attention_bwd.py, whose helpers are reused) at B 2, nH 3,
bf16 and lengths from the library's own tiles.  Where every query has one live key (S = 1) the oracle's dq and
dk are zeros and so is the bound: the kernels' dP has to equal delta bit for bit there.
TRLX_T5_ATTENTION_BWD_D256_PARITY_OUT=<file> writes the figures (profiles/t5_attention_bwd_d256_parity.json).
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
from test_gpu_t5_attention_bwd import bits, dev, train_call, same_bits, c_args

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TR = P.t5_attention_train
D = 256


def lib_tiles():
    t = [ctypes.c_int(0) for _ in range(4)]
    _lib.call("trlx_t5_attention_bwd_tiles_d", D, *[ctypes.byref(x) for x in t])
    return tuple(x.value for x in t)


DQ_Q, DQ_KV, DKV_K, DKV_Q = lib_tiles()
TILES = [P.t5_attention.tiles(D), (DQ_Q, DQ_KV), (DKV_Q, DKV_K)]
SIZES = CB.sizes(TILES)
CROSS = CB.cross_sizes(TILES)
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_ATTENTION_BWD_D256_PARITY_OUT")
    if path and _FIGURES:
        cases = [_FIGURES[k] for k in sorted(_FIGURES)]
        with open(path, "w") as f:
            json.dump({"rule": "per gradient: e_kernel <= 2 * e_torch + one bf16 ulp of max|oracle|",
                       "device": torch.cuda.get_device_name(0), "tiles_rows_columns": TILES,
                       "worst_ratio": max(c["ratio"] for c in cases), "cases": cases}, f, indent=1)


def run_case(mode, Tq, S, kind):
    """One parity case: the kernels on NaN-poisoned masked rows, the eager autograd on zeroed ones."""
    c = C.case(D, Tq, S, kind)
    mask = c["mask"]
    bidir, causal = mode == "encoder", mode == "decoder"
    dout = CB.make_dout(D, Tq, S)
    table64 = None if mode == "cross" else CB.table_from(c["W"], Tq, S, bidir)
    want = CB.oracle_grads(c["q"], c["k"], c["v"], dout, table64, mask, causal)
    q, mk, g = dev(c["q"], mask, dout)
    table = None if table64 is None else P.t5_relative_bias_offsets(c["W"].to(DEV), Tq, S, bidir)
    kp, vp = dev(C.poison(c["k"], mask), C.poison(c["v"], mask))
    got = train_call(q, kp, vp, table, mk, causal, g)
    assert torch.equal(bits(got["out"]), bits(P.t5_attention(q, kp, vp, bias=table, key_mask=mk, causal=causal)))
    for n, ref in (("dq", q), ("dk", kp), ("dv", vp)):
        assert got[n].dtype == torch.bfloat16 and got[n].shape == ref.shape and bool(torch.isfinite(got[n]).all()), n
    if mask is not None:
        gone = (mk == 0)[:, None, :, None]
        assert float(got["dk"].float().masked_select(gone).abs().sum()) == 0.0
        assert float(got["dv"].float().masked_select(gone).abs().sum()) == 0.0
    kz, vz = dev(C.poison(c["k"], mask, 0.0), C.poison(c["v"], mask, 0.0))
    figs = CB.judge(got, CB.eager_grads(q, kz, vz, g, table, mk, causal), want)
    for n, (e_k, e_t, lim) in figs.items():
        fig = dict(mode=mode, Tq=Tq, S=S, mask=kind, grad=n, e_torch=e_t, e_kernel=e_k, bound=lim,
                   ratio=e_k / lim if lim > 0 else (0.0 if e_k == 0 else float("inf")), max_abs=float(want[n].abs().max()))
        _FIGURES[(mode, Tq, S, kind, n)] = fig
        print(fig)
    for n, (e_k, e_t, lim) in figs.items():
        assert e_k <= lim, (n, figs)
    assert set(figs) == ({"dq", "dk", "dv"} if table is None else set(CB.GRADS))


@pytest.mark.parametrize("kind", C.MASKS)
@pytest.mark.parametrize("T", SIZES)
def test_encoder_parity(T, kind):
    run_case("encoder", T, T, kind)


@pytest.mark.parametrize("T", SIZES)
def test_decoder_causal_parity(T):
    run_case("decoder", T, T, "none")


@pytest.mark.parametrize("kind", C.MASKS)
@pytest.mark.parametrize("Tq,S", CROSS)
def test_cross_parity(Tq, S, kind):
    run_case("cross", Tq, S, kind)


# ------------------------------------------------------------------ checks no tolerance can hide
def encoder_setup(T, kind="holes"):
    c = C.case(D, T, T, kind)
    q, k, v, mk, W, g = dev(c["q"], c["k"], c["v"], c["mask"], c["W"], CB.make_dout(D, T, T))
    table = P.t5_relative_bias_offsets(W, T, T, True)
    return q, k, v, mk, table, g, train_call(q, k, v, table, mk, False, g)


def check_reproducible_strides_dbias():
    T = 2 * DKV_K + 3
    q, k, v, mk, table, g, ref = encoder_setup(T)
    assert same_bits(train_call(q, k, v, table, mk, False, g), ref)                     # a second run
    assert same_bits(train_call(q, k, v, table, mk, False, g, want_dbias=False), ref)   # the dbias=None path
    bthd = [x.transpose(1, 2).contiguous() for x in (q, k, v)]
    qkv = torch.cat([x.flatten(2) for x in bthd], dim=2).requires_grad_()               # a fused projection's slices
    inner = C.NH * D
    out = TR(*[qkv[:, :, i * inner:(i + 1) * inner] for i in range(3)], bias=table, key_mask=mk, n_heads=C.NH)
    assert torch.equal(bits(out), bits(ref["out"]))
    gq, = torch.autograd.grad(out, [qkv], g)
    for i, n in enumerate(("dq", "dk", "dv")):
        got = gq[:, :, i * inner:(i + 1) * inner].unflatten(2, (C.NH, D)).transpose(1, 2)
        assert torch.equal(bits(got), bits(ref[n])), n
    leaves = [x.clone().requires_grad_() for x in bthd]
    gs = torch.autograd.grad(TR(*leaves, bias=table, key_mask=mk, layout="bthd"), leaves, g)
    for x, n in zip(gs, ("dq", "dk", "dv")):
        assert torch.equal(bits(x.transpose(1, 2)), bits(ref[n])), n


def check_batch_row_alone():
    q, k, v, mk, table, g, ref = encoder_setup(DKV_K + 1, "left")
    alone = train_call(q[1:2], k[1:2], v[1:2], table, mk[1:2], False, g[1:2])
    for n in ("dq", "dk", "dv"):
        assert torch.equal(bits(alone[n][0]), bits(ref[n][1])), n


def check_fully_masked_row():
    q, k, v, mk, table, g, ref = encoder_setup(DQ_KV + 1, "right")
    mk0 = mk.clone()
    mk0[0] = 0
    got = train_call(q, C.poison(k, mk0), C.poison(v, mk0), table, mk0, False, g)
    for n in ("dq", "dk", "dv"):
        assert float(got[n][0].float().abs().max()) == 0.0 and bool(torch.isfinite(got[n]).all()), n
        assert torch.equal(bits(got[n][1]), bits(ref[n][1])), n
    assert bool(torch.isfinite(got["dbias"]).all())


def check_causal_range():
    """NaN in the q and dO rows below a key block leaves that block's dk / dv and the later dq rows their
    bits (those query tiles are not loaded for it); a later query perturbed leaves the keys past it theirs."""
    T, E = 200, 2 * DKV_K
    c = C.case(D, T, T)
    q, k, v, W, g = dev(c["q"], c["k"], c["v"], c["W"], CB.make_dout(D, T, T))
    table = P.t5_relative_bias_offsets(W, T, T, False)
    ref = train_call(q, k, v, table, None, True, g, want_dbias=False)
    q2, g2 = q.clone(), g.clone()
    q2[:, :, :E] = float("nan")
    g2[:, :E] = float("nan")
    got = train_call(q2, k, v, table, None, True, g2, want_dbias=False)
    for n in ("dk", "dv", "dq"):
        assert torch.equal(bits(got[n][:, :, E:]), bits(ref[n][:, :, E:])), n
    q3, g3 = q.clone(), g.clone()                                 # queries from E on perturbed: keys past the last one keep
    q3[:, :, E:E + 3] += 1.0                                      # nothing, keys before E + 3 change, dq below E keeps its bits
    got = train_call(q3, k, v, table, None, True, g3, want_dbias=False)
    assert torch.equal(bits(got["dq"][:, :, :E]), bits(ref["dq"][:, :, :E]))
    for n in ("dk", "dv"):
        assert torch.equal(bits(got[n][:, :, E + 3:]), bits(ref[n][:, :, E + 3:])), n


def check_c_entry_canaries():
    T = DKV_K + 1
    q, k, v, mk, table, g, ref = encoder_setup(T)
    inner, gap, pad = C.NH * D, 8, 16
    row = 3 * (inner + gap) + gap
    out = torch.empty(C.B, T, inner, dtype=torch.bfloat16, device=DEV)
    lse_buf = torch.full((C.B * C.NH * T + 2 * pad,), 7.0, device=DEV)
    lse = lse_buf[pad:pad + C.B * C.NH * T]
    fa = _lib.T5AttentionArgs(
        out=out.data_ptr(), o_stride_b=T * inner, o_stride_t=inner, o_stride_h=D, bias_by_offset=table.data_ptr(),
        key_mask=mk.data_ptr(), B=C.B, n_heads=C.NH, d_kv=D, Tq=T, S=T, dtype=_lib.BF16, causal=0,
        **{n: x.data_ptr() for n, x in (("q", q), ("k", k), ("v", v))},
        **{f"{n}_stride_{s}": x.stride(i) for n, x in (("q", q), ("k", k), ("v", v)) for s, i in (("b", 0), ("t", 2), ("h", 1))})
    _lib.call("trlx_t5_attention_fwd_lse", ctypes.byref(fa), lse.data_ptr(), _lib.stream_of(out))
    assert torch.equal(bits(out), bits(ref["out"]))
    buf = torch.full((C.B * T + 2, row), 7.0, dtype=torch.bfloat16, device=DEV)
    body = buf[1:1 + C.B * T]
    outs = [(body[:, gap + i * (inner + gap):], T * row, row) for i in range(3)]
    ws = torch.empty(_lib.query("trlx_t5_attention_bwd_workspace_bytes", C.B, C.NH, T), dtype=torch.uint8, device=DEV)
    a = c_args(q, k, v, out, g, lse, *outs, ws, D, T, T, bias_by_offset=table.data_ptr(), key_mask=mk.data_ptr())
    _lib.call("trlx_t5_attention_bwd", ctypes.byref(a), _lib.stream_of(out))
    torch.cuda.synchronize()
    assert bool((lse_buf[:pad] == 7.0).all()) and bool((lse_buf[pad + lse.numel():] == 7.0).all())
    assert bool((buf[0] == 7.0).all()) and bool((buf[-1] == 7.0).all())
    keep = torch.ones(row, dtype=torch.bool, device=DEV)
    for i, n in enumerate(("dq", "dk", "dv")):
        lo = gap + i * (inner + gap)
        keep[lo:lo + inner] = False
        assert torch.equal(bits(body[:, lo:lo + inner].reshape(C.B, T, C.NH, D).transpose(1, 2)), bits(ref[n])), n
    assert bool((body[:, keep] == 7.0).all())


def check_refused_calls():
    T = 9
    c = C.case(D, T, T)
    q, k, v, g = dev(c["q"], c["k"], c["v"], CB.make_dout(D, T, T))
    inner = C.NH * D
    out, lse = P.t5_attention(q, k, v), torch.zeros(C.B, C.NH, T, device=DEV)
    dq, dk, dv = (torch.full((C.B, T, inner), 7.0, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    ws = torch.empty(_lib.query("trlx_t5_attention_bwd_workspace_bytes", C.B, C.NH, T), dtype=torch.uint8, device=DEV)
    dense = [(x, T * inner, inner) for x in (dq, dk, dv)]
    for over in (dict(dtype=_lib.F32), dict(d_kv=96), dict(q=q.data_ptr() + 2)):
        with pytest.raises(ValueError, match="status 5"):
            _lib.call("trlx_t5_attention_bwd", ctypes.byref(c_args(q, k, v, out, g, lse, *dense, ws, D, T, T, **over)),
                      _lib.stream_of(out))
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in (dq, dk, dv))


def check_tiles():
    for d in (64, 128, 256):
        t = [ctypes.c_int(0) for _ in range(4)]
        _lib.call("trlx_t5_attention_bwd_tiles_d", d, *[ctypes.byref(x) for x in t])
        assert tuple(x.value for x in t) == TR.tiles(d)
    assert TR.tiles(64) == (TR.DQ_Q_TILE, TR.DQ_KV_TILE, TR.DKV_K_TILE, TR.DKV_Q_TILE)
    with pytest.raises(ValueError, match="status 5"):
        _lib.call("trlx_t5_attention_bwd_tiles_d", 96, None, None, None, None)


@pytest.mark.parametrize("check", [check_reproducible_strides_dbias, check_batch_row_alone, check_fully_masked_row,
                                   check_causal_range, check_c_entry_canaries, check_refused_calls, check_tiles],
                         ids=lambda f: f.__name__)
def test_exact(check):
    check()


def test_the_autograd_node_holds_nothing_of_size_tq_x_s():
    Bm, nH, T = 1, 2, 1024
    g0 = torch.Generator().manual_seed(5)
    q, k, v = ((torch.randn(Bm, nH, T, D, generator=g0) * D ** -0.25).to(torch.bfloat16).to(DEV).requires_grad_()
               for _ in range(3))
    W = torch.randn(C.NUM_BUCKETS, nH, generator=g0).to(DEV).requires_grad_()
    buckets = P.t5_relative_bias_buckets(T, T, True, device=DEV)
    dout = torch.randn(Bm, T, nH * D, generator=g0).to(torch.bfloat16).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = TR(q, k, v, bias=W.float()[buckets].t().contiguous(), key_mask=None)
    out.backward(dout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    score, own = Bm * nH * T * T * 2, 4 * Bm * nH * T * D * 2      # one bf16 score tensor; out and dq, dk, dv
    print(f"peak rise over forward + backward: {rise} bytes; one bf16 score tensor: {score}; out + gradients: {own}")
    assert all(x.grad is not None for x in (q, k, v, W))
    assert rise < score + own
