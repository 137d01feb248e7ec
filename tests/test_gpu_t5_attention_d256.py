"""T5's full-sequence attention at d_kv 256 on the GPU (csrc/t5_attention_d256.hip
k_t5_attention_d256, reached through trlx_t5_attention and t5_attention.t5_attention) against the
float64 oracle of tests/t5_attention_checks.py, under that file's rule, measured per case:
    max|kernel - f64| <= 2 * max|eager bf16 on the device - f64| + one bf16 ulp of max|f64|
B 2, nH 3, bf16.  Lengths from the kernel's own tiles, tiles(256): 1, around one KV tile, past one
Q tile, past two KV tiles, 200; masked K / V rows hold NaN for the kernel and zeros for eager.
Beside the rule, the checks no tolerance can hide.
TRLX_T5_ATTENTION_D256_PARITY_OUT=<file>: the measured figures are written there
(profiles/t5_attention_d256_parity.json is such a run)."""
import ctypes
import json
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D = 256
QT, KT = P.t5_attention.tiles(D)
_FIGURES = {}


def bits(x):
    return x.detach().contiguous().view(torch.int16).cpu()


def dev(*xs):
    return [None if x is None else x.to(DEV) for x in xs]


def c_args(qt, kt, vt, out, Tq, S, mk=None, **over):
    """TrlxT5AttentionArgs over [B, nH, T, d] operands and a [B, Tq, nH*d] out."""
    kw = dict(q=qt.data_ptr(), k=kt.data_ptr(), v=vt.data_ptr(), out=out.data_ptr(), bias_by_offset=None,
              key_mask=_lib.ptr(mk), B=C.B, n_heads=C.NH, d_kv=D, Tq=Tq, S=S, dtype=_lib.BF16, causal=0,
              o_stride_b=Tq * C.NH * D, o_stride_t=C.NH * D, o_stride_h=D)
    for n, x in (("q", qt), ("k", kt), ("v", vt)):
        kw[f"{n}_stride_b"], kw[f"{n}_stride_t"], kw[f"{n}_stride_h"] = x.stride(0), x.stride(2), x.stride(1)
    kw.update(over)
    return _lib.T5AttentionArgs(**kw)


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_ATTENTION_D256_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "e_kernel <= 2 * e_torch + one bf16 ulp of max|oracle|; e = max abs error against the "
                               "float64 oracle, e_torch = torch's eager route in bf16 on the device",
                       "device": torch.cuda.get_device_name(0), "d_kv": D, "Q_TILE": QT, "KV_TILE": KT,
                       "cases": [_FIGURES[k] for k in sorted(_FIGURES)]}, f, indent=1)


CASES = [("encoder", T, T, kind) for T in C.sizes(QT, KT) for kind in C.MASKS] \
    + [("decoder", T, T, "none") for T in C.sizes(QT, KT)] \
    + [("cross", Tq, S, kind) for Tq, S in C.cross_sizes(QT, KT) for kind in C.MASKS]


@pytest.mark.parametrize("mode,Tq,S,kind", CASES)
def test_parity(mode, Tq, S, kind):
    c = C.case(D, Tq, S, kind)
    mask, bidir, causal = c["mask"], mode == "encoder", mode == "decoder"
    W = None if mode == "cross" else c["W"]
    want = C.oracle(c["q"], c["k"], c["v"], W, bidir, mask=mask, causal=causal)
    q, mk, Wd = dev(c["q"], mask, W)
    table = None if W is None else P.t5_relative_bias_offsets(Wd, Tq, S, bidir)
    kp, vp = dev(C.poison(c["k"], mask), C.poison(c["v"], mask))
    if mode == "cross":   # the C entry itself: refused before d_kv 256 had a kernel
        got = torch.empty(C.B, Tq, C.NH * D, dtype=torch.bfloat16, device=DEV)
        _lib.call("trlx_t5_attention", ctypes.byref(c_args(q, kp, vp, got, Tq, S, mk)), _lib.stream_of(got))
    else:
        got = P.t5_attention(q, kp, vp, bias=table, key_mask=mk, causal=causal)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (C.B, Tq, C.NH * D) and got.is_contiguous()
    kz, vz = dev(C.poison(c["k"], mask, 0.0), C.poison(c["v"], mask, 0.0))
    e_k, e_t = C.max_err(got, want), C.max_err(C.eager(q, kz, vz, table, mk, causal), want)
    lim = C.bound(e_t, want)
    fig = dict(mode=mode, d_kv=D, Tq=Tq, S=S, mask=kind, e_torch=e_t, e_kernel=e_k, bound=lim, ratio=e_k / lim,
               max_abs=float(want.abs().max()))
    _FIGURES[(mode, Tq, S, kind)] = fig
    print(fig)
    assert torch.isfinite(got).all()
    assert e_k <= lim, fig


@pytest.mark.parametrize("check", ["layouts", "batch_row_alone", "fully_masked_row", "canary", "refused", "tiles"])
def test_exact(check):
    T = 2 * KT + 3 if check == "layouts" else QT + 1
    c = C.case(D, T, T, "holes" if check != "batch_row_alone" else "left")
    q, k, v, mk, W = dev(c["q"], c["k"], c["v"], c["mask"], c["W"])
    table = P.t5_relative_bias_offsets(W, T, T, True)
    kw = dict(bias=table, key_mask=mk)
    ref = P.t5_attention(q, k, v, **kw)
    inner = C.NH * D
    if check == "layouts":   # [B, T, nH, d], [B, T, nH*d] and a fused-qkv slice against [B, nH, T, d]
        bthd = [x.transpose(1, 2).contiguous() for x in (q, k, v)]
        assert torch.equal(bits(P.t5_attention(*bthd, layout="bthd", **kw)), bits(ref))
        flat = [x.flatten(2) for x in bthd]
        assert torch.equal(bits(P.t5_attention(*flat, n_heads=C.NH, **kw)), bits(ref))
        qkv = torch.cat(flat, dim=2)
        slices = [qkv[:, :, i * inner:(i + 1) * inner] for i in range(3)]
        assert not slices[1].is_contiguous()
        assert torch.equal(bits(P.t5_attention(*slices, n_heads=C.NH, **kw)), bits(ref))
    elif check == "batch_row_alone":
        alone = P.t5_attention(q[1:2], k[1:2], v[1:2], bias=table, key_mask=mk[1:2])
        assert torch.equal(bits(alone[0]), bits(ref[1]))
        assert torch.equal(bits(P.t5_attention(q, k, v, **kw)), bits(ref))
    elif check == "fully_masked_row":
        mk0 = mk.clone()
        mk0[0] = 0
        got = P.t5_attention(q, C.poison(k, mk0), C.poison(v, mk0), bias=table, key_mask=mk0)
        assert float(got[0].float().abs().max()) == 0.0
        assert torch.equal(bits(got[1]), bits(ref[1]))
    elif check == "canary":   # the C entry writes into the middle of a larger buffer
        pad = 4
        buf = torch.full((C.B * T + 2 * pad, inner), 7.0, dtype=torch.bfloat16, device=DEV)
        out = buf[pad:pad + C.B * T]
        _lib.call("trlx_t5_attention", ctypes.byref(c_args(q, k, v, out, T, T, mk)), _lib.stream_of(buf))
        torch.cuda.synchronize()
        assert bool((buf[:pad] == 7.0).all()) and bool((buf[pad + C.B * T:] == 7.0).all())
        assert torch.equal(bits(out.reshape(C.B, T, inner)), bits(P.t5_attention(q, k, v, key_mask=mk)))
    elif check == "refused":
        out = torch.full((C.B, T, inner), 7.0, dtype=torch.bfloat16, device=DEV)
        for over in (dict(q=q.data_ptr() + 2), dict(dtype=_lib.F32)):
            with pytest.raises(ValueError, match="status 5"):
                _lib.call("trlx_t5_attention", ctypes.byref(c_args(q, k, v, out, T, T, mk, **over)), _lib.stream_of(out))
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    else:
        for d in (64, 128, 256):
            q_tile, kv_tile = ctypes.c_int(0), ctypes.c_int(0)
            _lib.call("trlx_t5_attention_tiles_d", d, ctypes.byref(q_tile), ctypes.byref(kv_tile))
            assert (q_tile.value, kv_tile.value) == P.t5_attention.tiles(d)
        with pytest.raises(ValueError, match="status 5"):
            _lib.call("trlx_t5_attention_tiles_d", 96, None, None)
