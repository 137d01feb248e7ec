"""The T5 decode-step attention on the GPU (csrc/t5_decode_attn.hip k_t5_decode_attn,
trlx_t5_decode_attn, t5_decode.t5_decode_self_attention / t5_decode_cross_attention) against the
float64 oracle of tests/t5_decode_attn_checks.py.

Tolerance (measured, not fixed in advance): for every case e_torch = max|(a) - (b)|, torch's own
eager route in the input dtype on the device (matmul, add, fp32 softmax cast back, matmul) against
the oracle on the same inputs; the kernel must satisfy
    bf16   max|kernel - (b)| <= e_torch + one bf16 ulp of max|(b)|
    fp32   max|kernel - (b)| <= 4 * e_torch

Shapes: B 3, nH 5 (15 workgroups), d_kv in {64, 128}, bf16 and fp32, max_len 160.  Self-attention
t in {0, 7, 8, 9, 31, 32, 33, 127, 128, 129, 159}: around one wave-wide load of keys (8 at bf16
d_kv 64), around all 32 groups' first round, around the bucket saturation at distance 128, the
last column.  Cross-attention S in {1, 9, 33, 200} under no mask, right padding, left padding and
holes, the masked key and value rows holding NaN.  Beside the rule, checks no tolerance can hide:
cache columns bit for bit, NaN above t never read, strided operands give the contiguous bits, a
fully masked row gives exact zeros, a refused call leaves the output untouched.

TRLX_T5_DECODE_ATTN_PARITY_OUT=<file>: the measured figures are written there
(profiles/t5_decode_attn_parity.json is such a run).
"""
import ctypes
import json
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_decode_attn_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_CASES = {}
_TABLES = {}
_FIGURES = {}


def self_case(dtype, d):
    """The (dtype, d_kv) token stream, generated once and never modified."""
    if (dtype, d) not in _CASES:
        _CASES[(dtype, d)] = C.self_case(dtype, d)
        _TABLES[(dtype, d)] = P.t5_relative_bias_table(_CASES[(dtype, d)]["W"].to(DEV), C.MAX_LEN)
    return _CASES[(dtype, d)], _TABLES[(dtype, d)]


def bits(x):
    return x.detach().contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32).cpu()


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_DECODE_ATTN_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "bf16: e_kernel <= e_torch + one bf16 ulp of max|oracle|; fp32: e_kernel <= 4 * e_torch; "
                               "e = max abs error against the float64 oracle, e_torch = torch's eager route in the "
                               "input dtype on the device",
                       "device": torch.cuda.get_device_name(0),
                       "cases": [_FIGURES[k] for k in sorted(_FIGURES)]}, f, indent=1)


def judge(key, dtype, got, eager, want, **tags):
    e_k, e_t = C.max_err(got, want), C.max_err(eager, want)
    lim = C.bound(dtype, e_t, want)
    fig = dict(tags, dtype=C.dtype_name(dtype), e_torch=e_t, e_kernel=e_k, bound=lim, max_abs=float(want.abs().max()))
    _FIGURES[key] = fig
    print(fig)
    assert torch.isfinite(got).all()
    assert e_k <= lim, fig


def filled_cache(c, dtype, d, t, above=0.0):
    """A cache holding the stream's columns below t, `above` everywhere from t on."""
    cache = P.T5DecodeKVCache(C.B, C.NH, d, C.MAX_LEN, dtype, DEV)
    for dst, src in ((cache.k, c["K"]), (cache.v, c["V"])):
        dst.fill_(above)
        dst[:, :, :t] = src[:, :, :t].to(DEV)
    return cache


def oracle_self(c, t, W):
    K, V = c["K"].double().clone(), c["V"].double().clone()
    K[:, :, t:] = 0
    V[:, :, t:] = 0
    return C.oracle_self_step(c["Q"][:, :, t], c["K"][:, :, t], c["V"][:, :, t], K, V, t, W)


# ------------------------------------------------------------------ self-attention
@pytest.mark.parametrize("t", C.SELF_T)
@pytest.mark.parametrize("d", C.D_KVS)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dtype_name)
def test_self_attention_parity(dtype, d, t):
    c, table = self_case(dtype, d)
    cache = filled_cache(c, dtype, d, t)
    q, kn, vn = (c[n][:, :, t].to(DEV) for n in "QKV")
    got = P.t5_decode_self_attention(q, kn, vn, cache, t, table)
    assert got.dtype == dtype and tuple(got.shape) == (C.B, C.NH * d) and got.is_contiguous()
    eager = C.eager_self(q, cache.k, cache.v, t, table)    # after the call: column t is in the cache
    judge(("self", C.dtype_name(dtype), d, t), dtype, got, eager, oracle_self(c, t, c["W"]), mode="self", d_kv=d, t=t)


@pytest.mark.parametrize("dtype,d,t", [(torch.bfloat16, 64, 33), (torch.float32, 128, 9)], ids=str)
def test_self_attention_without_a_bias(dtype, d, t):
    c, _ = self_case(dtype, d)
    cache = filled_cache(c, dtype, d, t)
    q, kn, vn = (c[n][:, :, t].to(DEV) for n in "QKV")
    got = P.t5_decode_self_attention(q, kn, vn, cache, t)
    judge(("self_nobias", C.dtype_name(dtype), d, t), dtype, got, C.eager_self(q, cache.k, cache.v, t),
          oracle_self(c, t, None), mode="self, no bias", d_kv=d, t=t)


@pytest.mark.parametrize("dtype,d,t", [(torch.bfloat16, 64, 33), (torch.bfloat16, 128, 8), (torch.float32, 64, 0),
                                       (torch.float32, 128, 159)], ids=str)
def test_cache_after_the_call_and_nan_above_t(dtype, d, t):
    """Column t is k_new / v_new bit for bit, every other column keeps its bits; columns above t
    full of NaN are never read: the output is finite and has the bits of the run over zeros."""
    c, table = self_case(dtype, d)
    q, kn, vn = (c[n][:, :, t].to(DEV) for n in "QKV")
    outs = []
    for above in (0.0, float("nan")):
        cache = filled_cache(c, dtype, d, t, above)
        before_k, before_v = bits(cache.k), bits(cache.v)
        outs.append(P.t5_decode_self_attention(q, kn, vn, cache, t, table))
        for now, before, new in ((cache.k, before_k, kn), (cache.v, before_v, vn)):
            now = bits(now)
            assert torch.equal(now[:, :, t], bits(new))
            assert torch.equal(now[:, :, :t], before[:, :, :t]) and torch.equal(now[:, :, t + 1:], before[:, :, t + 1:])
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 64), (torch.float32, 128)], ids=str)
def test_strided_slices_of_a_fused_projection(dtype, d):
    """q, k_new, v_new as the three slices of one [B, 3·nH·d_kv] tensor, and as HF's [B, nH, 1, d_kv]
    views of it: read in place, the contiguous run's bits."""
    t = 33
    c, table = self_case(dtype, d)
    inner = C.NH * d
    q, kn, vn = (c[n][:, :, t].reshape(C.B, inner).to(DEV) for n in "QKV")
    want = P.t5_decode_self_attention(q, kn, vn, filled_cache(c, dtype, d, t), t, table)
    qkv = torch.cat([q, kn, vn], dim=1)
    sl = [qkv[:, i * inner:(i + 1) * inner] for i in range(3)]
    assert all(s.stride(0) == 3 * inner and not s.is_contiguous() for s in sl)
    views = [s.view(C.B, 1, C.NH, d).transpose(1, 2) for s in sl]
    for ops in (sl, views):
        cache = filled_cache(c, dtype, d, t)
        got = P.t5_decode_self_attention(*ops, cache, t, table)
        assert torch.equal(bits(got), bits(want))
        assert torch.equal(bits(cache.k[:, :, t]), bits(kn.view(C.B, C.NH, d)))
        assert torch.equal(bits(cache.v[:, :, t]), bits(vn.view(C.B, C.NH, d)))


@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 64), (torch.float32, 64), (torch.bfloat16, 128)], ids=str)
def test_decode_loop_from_an_empty_cache(dtype, d):
    """48 steps from an empty cache; the oracle steps the same inputs with its own float64 cache."""
    c, table = self_case(dtype, d)
    cache = P.T5DecodeKVCache(C.B, C.NH, d, C.MAX_LEN, dtype, DEV)
    K = torch.zeros(C.B, C.NH, C.MAX_LEN, d, dtype=torch.float64)
    V = torch.zeros_like(K)
    Q, Kn, Vn = (c[n].to(DEV) for n in "QKV")
    got, eager, want = [], [], []
    for t in range(C.LOOP_STEPS):
        got.append(P.t5_decode_self_attention(Q[:, :, t], Kn[:, :, t], Vn[:, :, t], cache, t, table))
        eager.append(C.eager_self(Q[:, :, t], cache.k, cache.v, t, table))
        want.append(C.oracle_self_step(c["Q"][:, :, t], c["K"][:, :, t], c["V"][:, :, t], K, V, t, c["W"]))
    judge(("loop", C.dtype_name(dtype), d), dtype, torch.stack(got), torch.stack(eager), torch.stack(want),
          mode="self, 48-step loop", d_kv=d)
    assert torch.equal(bits(cache.k[:, :, :C.LOOP_STEPS]), bits(Kn[:, :, :C.LOOP_STEPS]))
    assert float(cache.k[:, :, C.LOOP_STEPS:].abs().max()) == 0.0


# ------------------------------------------------------------------ cross-attention
@pytest.mark.parametrize("kind", C.MASKS)
@pytest.mark.parametrize("S", C.CROSS_S)
@pytest.mark.parametrize("d", C.D_KVS)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dtype_name)
def test_cross_attention_parity(dtype, d, S, kind):
    c = C.cross_case(dtype, d, S, kind)
    mask = c["mask"]
    q = c["q"].to(DEV)
    Kp, Vp = C.poison(c["K"], mask).to(DEV), C.poison(c["V"], mask).to(DEV)    # NaN in the masked rows
    mdev = None if mask is None else mask.to(DEV)
    got = P.t5_decode_cross_attention(q, Kp, Vp, mdev)
    assert got.dtype == dtype and tuple(got.shape) == (C.B, C.NH * d)
    eager = C.eager_cross(q, c["K"].to(DEV), c["V"].to(DEV), mdev)
    judge(("cross", C.dtype_name(dtype), d, S, kind), dtype, got, eager, C.oracle_cross(c["q"], Kp.cpu(), Vp.cpu(), mask),
          mode="cross", d_kv=d, S=S, mask=kind)


@pytest.mark.parametrize("dtype,d,S", [(torch.bfloat16, 64, 33), (torch.float32, 128, 9), (torch.bfloat16, 128, 200)],
                         ids=str)
def test_fully_masked_row_gives_zeros_and_leaves_its_neighbours(dtype, d, S):
    c = C.cross_case(dtype, d, S, "holes")
    q = c["q"].to(DEV)
    mask = c["mask"].clone()
    ref = P.t5_decode_cross_attention(q, C.poison(c["K"], mask).to(DEV), C.poison(c["V"], mask).to(DEV), mask.to(DEV))
    mask[1] = 0
    got = P.t5_decode_cross_attention(q, C.poison(c["K"], mask).to(DEV), C.poison(c["V"], mask).to(DEV), mask.to(DEV))
    assert torch.equal(bits(got[1]), torch.zeros_like(bits(got[1])))
    assert torch.equal(bits(got[0]), bits(ref[0])) and torch.equal(bits(got[2]), bits(ref[2]))
    assert float(ref[1].abs().max()) > 0.0


# ------------------------------------------------------------------ refusals
def _raw_args(dtype, d, **over):
    """A valid raw self-attention call over device buffers; `out` holds a pattern."""
    inner = C.NH * d
    x = torch.randn(C.B, inner, device=DEV).to(dtype)
    cache = P.T5DecodeKVCache(C.B, C.NH, d, C.MAX_LEN, dtype, DEV)
    out = torch.full((C.B, C.NH * 128), 7.0, dtype=dtype, device=DEV)
    kw = dict(q=x.data_ptr(), ldq=inner, k_new=x.data_ptr(), ldk=inner, v_new=x.data_ptr(), ldv=inner,
              k=cache.k.data_ptr(), v=cache.v.data_ptr(), bias_by_distance=None, key_mask=None, out=out.data_ptr(),
              B=C.B, n_heads=C.NH, d_kv=d, max_len=C.MAX_LEN, t=3, dtype=_lib.dtype_code(x), mode=_lib.T5_ATTN_SELF)
    kw.update(over)
    return _lib.T5DecodeAttnArgs(**kw), out, cache, x


@pytest.mark.parametrize("over", [dict(d_kv=96), dict(t=C.MAX_LEN), dict(ldq=C.NH * 64 - 8)], ids=str)
def test_refusals_raise_and_leave_the_output_untouched(over):
    a, out, cache, x = _raw_args(torch.bfloat16, 64, **over)
    with pytest.raises(ValueError, match="status 5"):
        _lib.call("trlx_t5_decode_attn", ctypes.byref(a), _lib.stream_of(out))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(cache.k.abs().max()) == 0.0 and float(cache.v.abs().max()) == 0.0
    # the same record with the offending field put right runs and writes
    a, out, cache, x = _raw_args(torch.bfloat16, 64)
    _lib.call("trlx_t5_decode_attn", ctypes.byref(a), _lib.stream_of(out))
    torch.cuda.synchronize()
    assert not bool((out.view(-1)[:C.B * C.NH * 64] == 7.0).all())
    assert torch.equal(bits(cache.k[:, :, 3]), bits(x.view(C.B, C.NH, 64)))


def test_python_entry_refuses_t_at_max_len():
    c, table = self_case(torch.bfloat16, 64)
    cache = P.T5DecodeKVCache(C.B, C.NH, 64, 8, torch.bfloat16, DEV)
    q = c["Q"][:, :, 0].to(DEV)
    with pytest.raises(ValueError, match="outside"):
        P.t5_decode_self_attention(q, q, q, cache, 8)
    assert float(cache.k.abs().max()) == 0.0
