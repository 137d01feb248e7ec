"""T5's full-sequence attention on the GPU (csrc/t5_attention.hip k_t5_attention, trlx_t5_attention,
t5_attention.t5_attention) against the float64 oracle of tests/t5_attention_checks.py.

Tolerance (measured, not fixed in advance): for every case e_torch = max|(a) - (b)|, torch's own
eager route in bf16 on the device (matmul, materialised bias plus additive mask, fp32 softmax cast
back, matmul) against the oracle on the same inputs; the kernel must satisfy
    max|kernel - (b)| <= 2 * e_torch + one bf16 ulp of max|(b)|
(tests/test_t5_attention_cpu.py shows a wrong bias index, a dropped key and an off-by-one causal
boundary more than 10x outside it).

Shapes: B 2, nH 3, bf16, d_kv in {64, 128}.  Encoder and decoder-causal lengths: 1, around one KV
tile, past one Q tile, past two KV tiles, 200; the encoder under no mask, right padding, left
padding and holes with the masked K and V rows holding NaN.  Cross: (Tq, S) in {(1, 200),
(Q_TILE + 1, 1), (48, 2 KV_TILE + 3), (130, 33)} under the same masks.  Beside the rule, checks no
tolerance can hide: strided operands give the contiguous bits, a batch row alone gives its bits in
the batch, a fully masked row gives exact zeros, a causal call does not read above the diagonal's
tiles, canary rows around `out` stay intact, a refused call leaves `out` untouched, the
[B, nH, S, d] keys handed on to the decode kernel are read in place by both.

TRLX_T5_ATTENTION_PARITY_OUT=<file>: the measured figures are written there
(profiles/t5_attention_parity.json is such a run).
"""
import ctypes
import json
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C
import t5_decode_attn_checks as CD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
QT, KT = P.t5_attention.Q_TILE, P.t5_attention.KV_TILE
SIZES = C.sizes(QT, KT)
CROSS = C.cross_sizes(QT, KT)
_FIGURES = {}
print(f"t5_attention tiles: Q_TILE {QT}, KV_TILE {KT}")


def bits(x):
    return x.detach().contiguous().view(torch.int16).cpu()


def dev(*xs):
    return [None if x is None else x.to(DEV) for x in xs]


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_ATTENTION_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "e_kernel <= 2 * e_torch + one bf16 ulp of max|oracle|; e = max abs error against the "
                               "float64 oracle, e_torch = torch's eager route in bf16 on the device",
                       "device": torch.cuda.get_device_name(0), "Q_TILE": QT, "KV_TILE": KT,
                       "cases": [_FIGURES[k] for k in sorted(_FIGURES)]}, f, indent=1)


def judge(key, got, eager, want, **tags):
    e_k, e_t = C.max_err(got, want), C.max_err(eager, want)
    lim = C.bound(e_t, want)
    fig = dict(tags, e_torch=e_t, e_kernel=e_k, bound=lim, ratio=e_k / lim, max_abs=float(want.abs().max()))
    _FIGURES[key] = fig
    print(fig)
    assert torch.isfinite(got).all()
    assert e_k <= lim, fig


def run_case(mode, d, Tq, S, kind):
    """One parity case: the kernel on NaN-poisoned masked rows, the eager route on zeroed ones."""
    c = C.case(d, Tq, S, kind)
    mask = c["mask"]
    bidir = mode == "encoder"
    causal = mode == "decoder"
    W = None if mode == "cross" else c["W"]
    want = C.oracle(c["q"], c["k"], c["v"], W, bidir, mask=mask, causal=causal)
    q, mk, Wd = dev(c["q"], mask, W)
    table = None if W is None else P.t5_relative_bias_offsets(Wd, Tq, S, bidir)
    kp, vp = dev(C.poison(c["k"], mask), C.poison(c["v"], mask))
    got = P.t5_attention(q, kp, vp, bias=table, key_mask=mk, causal=causal)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (C.B, Tq, C.NH * d) and got.is_contiguous()
    kz, vz = dev(C.poison(c["k"], mask, 0.0), C.poison(c["v"], mask, 0.0))
    eager = C.eager(q, kz, vz, table, mk, causal)
    judge((mode, d, Tq, S, kind), got, eager, want, mode=mode, d_kv=d, Tq=Tq, S=S, mask=kind)


def test_tiles_match_the_library():
    q_tile, kv_tile = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("trlx_t5_attention_tiles", ctypes.byref(q_tile), ctypes.byref(kv_tile))
    assert (q_tile.value, kv_tile.value) == (QT, KT)


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
def encoder_call(d, T, kind="holes"):
    c = C.case(d, T, T, kind)
    q, k, v, mk, W = dev(c["q"], c["k"], c["v"], c["mask"], c["W"])
    table = P.t5_relative_bias_offsets(W, T, T, True)
    return c, q, k, v, mk, table, P.t5_attention(q, k, v, bias=table, key_mask=mk)


@pytest.mark.parametrize("d", C.D_KVS)
def test_strided_operands_give_the_contiguous_bits(d):
    T = 2 * KT + 3
    c, q, k, v, mk, table, ref = encoder_call(d, T)
    kw = dict(bias=table, key_mask=mk)
    bthd = [x.transpose(1, 2).contiguous() for x in (q, k, v)]                # [B, T, nH, d]
    assert torch.equal(bits(P.t5_attention(*bthd, layout="bthd", **kw)), bits(ref))
    assert torch.equal(bits(P.t5_attention(*[x.transpose(1, 2) for x in bthd], **kw)), bits(ref))   # HF's view
    flat = [x.flatten(2) for x in bthd]                                       # [B, T, nH*d]
    assert torch.equal(bits(P.t5_attention(*flat, n_heads=C.NH, **kw)), bits(ref))
    qkv = torch.cat(flat, dim=2)                                              # a fused [B, T, 3*nH*d] projection
    inner = C.NH * d
    slices = [qkv[:, :, i * inner:(i + 1) * inner] for i in range(3)]
    ptr = qkv.data_ptr()
    assert torch.equal(bits(P.t5_attention(*slices, n_heads=C.NH, **kw)), bits(ref))
    assert qkv.data_ptr() == ptr and not slices[1].is_contiguous()
    odd = torch.zeros(C.B, C.NH, T, d + 4, dtype=torch.bfloat16, device=DEV)  # a stride the kernel refuses:
    odd[..., :d] = q                                                          # copied once, same bits
    assert torch.equal(bits(P.t5_attention(odd[..., :d], k, v, **kw)), bits(ref))


@pytest.mark.parametrize("d", C.D_KVS)
def test_a_batch_row_alone_gives_its_bits_in_the_batch(d):
    T = QT + 1
    c, q, k, v, mk, table, ref = encoder_call(d, T, "left")
    alone = P.t5_attention(q[1:2], k[1:2], v[1:2], bias=table, key_mask=mk[1:2])
    assert torch.equal(bits(alone[0]), bits(ref[1]))
    again = P.t5_attention(q, k, v, bias=table, key_mask=mk)
    assert torch.equal(bits(again), bits(ref))


@pytest.mark.parametrize("d", C.D_KVS)
def test_a_fully_masked_row_gives_exact_zeros(d):
    T = KT + 1
    c, q, k, v, mk, table, ref = encoder_call(d, T, "right")
    mk0 = mk.clone()
    mk0[0] = 0
    k0, v0 = C.poison(k, mk0), C.poison(v, mk0)
    got = P.t5_attention(q, k0, v0, bias=table, key_mask=mk0)
    assert float(got[0].float().abs().max()) == 0.0
    assert torch.equal(bits(got[1]), bits(ref[1]))


@pytest.mark.parametrize("d", C.D_KVS)
def test_a_causal_call_reads_nothing_above_its_tiles(d):
    """Rows [0, i] keep their bits when the K / V rows above i change: NaN above a Q-tile edge (those
    tiles are not loaded), other finite values above a KV-tile edge inside a Q tile (p is exactly 0)."""
    T = 200
    c = C.case(d, T, T)
    q, k, v, W = dev(c["q"], c["k"], c["v"], c["W"])
    table = P.t5_relative_bias_offsets(W, T, T, False)
    ref = P.t5_attention(q, k, v, bias=table, causal=True)
    for i, fill in ((QT - 1, float("nan")), (KT - 1, 3.0), (KT, -2.0)):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, i + 1:] = fill
        v2[:, :, i + 1:] = fill
        got = P.t5_attention(q, k2, v2, bias=table, causal=True)
        assert torch.equal(bits(got[:, :i + 1]), bits(ref[:, :i + 1])), i


@pytest.mark.parametrize("Tq,S", [(1, 1), (KT - 1, KT - 1), (KT + 1, KT + 1), (QT + 1, 1), (QT + 1, QT + 1), (48, 2 * KT + 3)])
@pytest.mark.parametrize("d", C.D_KVS)
def test_canary_rows_around_out_stay_intact(d, Tq, S):
    """The C entry writes into the middle of a larger buffer: the rows before and after keep their bits."""
    c = C.case(d, Tq, S, "holes")
    q, k, v, mk = dev(c["q"], c["k"], c["v"], c["mask"])
    inner, pad = C.NH * d, 4
    buf = torch.full((C.B * Tq + 2 * pad, inner), 7.0, dtype=torch.bfloat16, device=DEV)
    out = buf[pad:pad + C.B * Tq]
    a = _lib.T5AttentionArgs(
        q=q.data_ptr(), q_stride_b=q.stride(0), q_stride_t=q.stride(2), q_stride_h=q.stride(1),
        k=k.data_ptr(), k_stride_b=k.stride(0), k_stride_t=k.stride(2), k_stride_h=k.stride(1),
        v=v.data_ptr(), v_stride_b=v.stride(0), v_stride_t=v.stride(2), v_stride_h=v.stride(1),
        out=out.data_ptr(), o_stride_b=Tq * inner, o_stride_t=inner, o_stride_h=d, bias_by_offset=None,
        key_mask=mk.data_ptr(), B=C.B, n_heads=C.NH, d_kv=d, Tq=Tq, S=S, dtype=_lib.BF16, causal=0)
    _lib.call("trlx_t5_attention", ctypes.byref(a), _lib.stream_of(buf))
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 7.0).all()) and bool((buf[pad + C.B * Tq:] == 7.0).all())
    want = P.t5_attention(q, k, v, key_mask=mk)
    assert torch.equal(bits(out.reshape(C.B, Tq, inner)), bits(want))


def test_a_refused_c_call_leaves_out_untouched():
    d, T = 64, 9
    c = C.case(d, T, T)
    q, k, v = dev(c["q"], c["k"], c["v"])
    out = torch.full((C.B, T, C.NH * d), 7.0, dtype=torch.bfloat16, device=DEV)

    def args(**over):
        kw = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), out=out.data_ptr(), bias_by_offset=None, key_mask=None,
                  B=C.B, n_heads=C.NH, d_kv=d, Tq=T, S=T, dtype=_lib.BF16, causal=0,
                  o_stride_b=T * C.NH * d, o_stride_t=C.NH * d, o_stride_h=d)
        for n, x in (("q", q), ("k", k), ("v", v)):
            kw[f"{n}_stride_b"], kw[f"{n}_stride_t"], kw[f"{n}_stride_h"] = x.stride(0), x.stride(2), x.stride(1)
        kw.update(over)
        return _lib.T5AttentionArgs(**kw)

    for over in (dict(dtype=_lib.F32), dict(d_kv=96), dict(q_stride_t=d + 4), dict(q=q.data_ptr() + 2),
                 dict(causal=1, S=T - 1), dict(Tq=1 << 31), dict(o_stride_t=d)):
        with pytest.raises(ValueError, match="status 5"):
            _lib.call("trlx_t5_attention", ctypes.byref(args(**over)), _lib.stream_of(out))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _lib.call("trlx_t5_attention", ctypes.byref(args()), _lib.stream_of(out))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(P.t5_attention(q, k, v)))


@pytest.mark.parametrize("kind", ["none", "left"])
@pytest.mark.parametrize("d", C.D_KVS)
def test_the_keys_are_handed_on_to_the_decode_kernel_in_place(d, kind):
    """Cross-attention at Tq 1 over contiguous [B, nH, S, d] k / v: this kernel and
    t5_decode_cross_attention read the same tensors, each within its own rule."""
    S = 200
    c = C.case(d, 1, S, kind)
    mask = c["mask"]
    want = C.oracle(c["q"], c["k"], c["v"], mask=mask)                                     # [B, 1, nH*d]
    q, mk = dev(c["q"], mask)
    kp, vp = dev(C.poison(c["k"], mask), C.poison(c["v"], mask))
    ptrs = (kp.data_ptr(), vp.data_ptr())
    got = P.t5_attention(q, kp, vp, key_mask=mk)
    dec = P.t5_decode_cross_attention(q[:, :, 0], kp, vp, mk)
    assert (kp.data_ptr(), vp.data_ptr()) == ptrs and kp.is_contiguous()
    kz, vz = dev(C.poison(c["k"], mask, 0.0), C.poison(c["v"], mask, 0.0))
    e_t = C.max_err(C.eager(q, kz, vz, None, mk), want)
    assert C.max_err(got, want) <= C.bound(e_t, want)
    e_td = CD.max_err(CD.eager_cross(q[:, :, 0], kz, vz, mk), want[:, 0])
    assert CD.max_err(dec, want[:, 0]) <= CD.bound(torch.bfloat16, e_td, want[:, 0])
