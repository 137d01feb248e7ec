"""The live-row skip of the decode attention on the GPU (trlx_t5_decode_attn_live, the LIVE
instantiations of k_t5_decode_attn; t5_decode_self_attention / t5_decode_cross_attention(live=))
against the entries without it.

Every comparison is equality of the raw bits: a live row runs the existing kernel's code.  The q /
k_new / v_new of a skipped row are NaN and its cache column holds a sentinel, so anything read from
them into an output would show."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_rollout_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = (torch.bfloat16, torch.float32)
B, NH, MAX_LEN = 4, 3, 70
SELF_T = (0, 1, 63, 64, 69)
CROSS_S = (1, 63, 64, 65, 130)
LIVE = ([1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 7])
_CASES = {}


def case(dtype, d):
    """The inputs of one (dtype, d_kv), made once and never modified."""
    if (dtype, d) not in _CASES:
        g = torch.Generator().manual_seed(5200 + d + (1 if dtype == torch.float32 else 0))
        inner = NH * d
        qkv = (torch.randn(B, 3 * inner, generator=g) * d ** -0.25).to(dtype).to(DEV)
        K = (torch.randn(B, NH, MAX_LEN, d, generator=g) * d ** -0.25).to(dtype).to(DEV)
        Vv = torch.randn(B, NH, MAX_LEN, d, generator=g).to(dtype).to(DEV)
        table = P.t5_relative_bias_table(torch.randn(32, NH, generator=g).to(DEV), MAX_LEN)
        S = max(CROSS_S)
        k_enc = (torch.randn(B, NH, S, d, generator=g) * d ** -0.25).to(dtype).to(DEV)
        v_enc = torch.randn(B, NH, S, d, generator=g).to(dtype).to(DEV)
        mask = (torch.rand(B, S, generator=g) > 0.3).to(torch.int64)
        mask[:, 0] = 1
        mask[1, 5:9] = 0                                       # holes
        _CASES[(dtype, d)] = dict(qkv=qkv, K=K, V=Vv, table=table, inner=inner, k_enc=k_enc, v_enc=v_enc,
                                  mask=mask.to(DEV))
    return _CASES[(dtype, d)]


def new_cache(c, dtype, d, t):
    """The stream's columns below t, the guard from column t on."""
    cache = P.T5DecodeKVCache(B, NH, d, MAX_LEN, dtype, DEV)
    for dst, src in ((cache.k, c["K"]), (cache.v, c["V"])):
        dst.fill_(C.GUARD)
        dst[:, :, :t] = src[:, :, :t]
    return cache


def poisoned(x, live):
    """x with the rows of live == 0 set to NaN."""
    x = x.clone()
    x[live == 0] = float("nan")
    return x


@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("dtype", DTYPES, ids=C.name)
def test_self_attention_skips_dead_rows_and_keeps_live_rows(dtype, d):
    c = case(dtype, d)
    inner = c["inner"]
    q, kn, vn = (c["qkv"][:, i * inner:(i + 1) * inner] for i in range(3))
    clock = P.T5DecodeClock(MAX_LEN, DEV)
    for t in SELF_T:
        ref = new_cache(c, dtype, d, t)
        want = P.t5_decode_self_attention(q, kn, vn, ref, t, c["table"])
        assert torch.isfinite(want.float()).all()
        for pattern in LIVE:
            live = torch.tensor(pattern, dtype=torch.int64, device=DEV)
            on = live != 0
            qkv = poisoned(c["qkv"], live)                     # a fused projection: q / k_new / v_new are its slices
            pq, pk, pv = (qkv[:, i * inner:(i + 1) * inner] for i in range(3))
            host = new_cache(c, dtype, d, t)
            got = P.t5_decode_self_attention(pq, pk, pv, host, t, c["table"], live=live)
            assert C.same(got[on], want[on]), (t, pattern, "live rows")
            assert C.same(got[~on], torch.zeros_like(got[~on])), (t, pattern, "dead rows")
            for mine, theirs in ((host.k, ref.k), (host.v, ref.v)):
                assert C.same(mine[on], theirs[on]), (t, pattern, "cache of live rows")
                skipped = mine[~on]
                assert C.same(skipped[:, :, t:], torch.full_like(skipped[:, :, t:], C.GUARD)), (t, pattern, "sentinel")
                assert C.same(skipped[:, :, :t], c["K" if mine is host.k else "V"][~on][:, :, :t])
            # the clock form is the host form
            dev = new_cache(c, dtype, d, t)
            clock.record[_lib.CLOCK_T] = t
            got_c = P.t5_decode_self_attention(pq, pk, pv, dev, clock, c["table"], live=live)
            assert C.same(got_c, got) and C.same(dev.k, host.k) and C.same(dev.v, host.v), (t, pattern, "clock")
            assert live.tolist() == pattern and clock.t == t


@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("dtype", DTYPES, ids=C.name)
def test_cross_attention_skips_dead_rows_and_keeps_live_rows(dtype, d):
    c = case(dtype, d)
    q = c["qkv"][:, :c["inner"]]
    for S in CROSS_S:
        k_enc, v_enc = c["k_enc"][:, :, :S].contiguous(), c["v_enc"][:, :, :S].contiguous()
        for mask in (c["mask"][:, :S].contiguous(), None):
            want = P.t5_decode_cross_attention(q, k_enc, v_enc, mask)
            for pattern in LIVE:
                live = torch.tensor(pattern, dtype=torch.int64, device=DEV)
                on = live != 0
                pq = poisoned(c["qkv"], live)[:, :c["inner"]]
                pk, pv = poisoned(k_enc, live), poisoned(v_enc, live)
                got = P.t5_decode_cross_attention(pq, pk, pv, mask, live=live)
                assert C.same(got[on], want[on]), (S, pattern, mask is None, "live rows")
                assert C.same(got[~on], torch.zeros_like(got[~on])), (S, pattern, mask is None, "dead rows")


def test_a_dead_clock_step_with_live_rows_is_the_dead_step():
    dtype, d = torch.bfloat16, 64
    c = case(dtype, d)
    inner = c["inner"]
    q, kn, vn = (c["qkv"][:, i * inner:(i + 1) * inner] for i in range(3))
    live = torch.tensor([1, 0, 1, 1], dtype=torch.int64, device=DEV)
    for T, t in ((MAX_LEN, MAX_LEN), (MAX_LEN, -1), (5, 5)):
        clock = P.T5DecodeClock(T, DEV)
        clock.record[_lib.CLOCK_T] = t
        cache = new_cache(c, dtype, d, 0)
        out = P.t5_decode_self_attention(q, kn, vn, cache, clock, c["table"], live=live)
        assert C.same(out, torch.zeros_like(out))
        assert C.same(cache.k, torch.full_like(cache.k, C.GUARD)) and C.same(cache.v, torch.full_like(cache.v, C.GUARD))


def test_live_none_still_takes_the_old_entries(monkeypatch):
    dtype, d = torch.bfloat16, 64
    c = case(dtype, d)
    inner = c["inner"]
    q, kn, vn = (c["qkv"][:, i * inner:(i + 1) * inner] for i in range(3))
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    a, b = new_cache(c, dtype, d, 9), new_cache(c, dtype, d, 9)
    out_none = P.t5_decode_self_attention(q, kn, vn, a, 9, c["table"], live=None)
    out_old = P.t5_decode_self_attention(q, kn, vn, b, 9, c["table"])
    k_enc, v_enc = c["k_enc"][:, :, :65].contiguous(), c["v_enc"][:, :, :65].contiguous()
    x_none = P.t5_decode_cross_attention(q, k_enc, v_enc, None, live=None)
    clock = P.T5DecodeClock(MAX_LEN, DEV)
    P.t5_decode_self_attention(q, kn, vn, new_cache(c, dtype, d, 0), clock, c["table"], live=None)
    assert [n for n in called if "decode_attn" in n] == ["trlx_t5_decode_attn"] * 3 + ["trlx_t5_decode_attn_dev"]
    assert C.same(out_none, out_old) and C.same(a.k, b.k) and C.same(a.v, b.v)
    ones = torch.ones(B, dtype=torch.int64, device=DEV)
    assert C.same(P.t5_decode_cross_attention(q, k_enc, v_enc, None, live=ones), x_none)
    assert called[-1] == "trlx_t5_decode_attn_live"


def test_refusals():
    dtype, d = torch.bfloat16, 64
    c = case(dtype, d)
    inner = c["inner"]
    q, kn, vn = (c["qkv"][:, i * inner:(i + 1) * inner] for i in range(3))
    cache = new_cache(c, dtype, d, 0)
    k_enc, v_enc = c["k_enc"][:, :, :8].contiguous(), c["v_enc"][:, :, :8].contiguous()
    bad = (torch.ones(B, dtype=torch.int64), torch.ones(B, dtype=torch.int32, device=DEV),
           torch.ones(B + 1, dtype=torch.int64, device=DEV), torch.ones(2 * B, dtype=torch.int64, device=DEV)[::2])
    for live in bad:
        with pytest.raises(ValueError, match="live"):
            P.t5_decode_self_attention(q, kn, vn, cache, 0, c["table"], live=live)
        with pytest.raises(ValueError, match="live"):
            P.t5_decode_cross_attention(q, k_enc, v_enc, live=live)
    # the C entry
    out = torch.full((B, inner), C.GUARD, dtype=dtype, device=DEV)
    live = torch.ones(B + 1, dtype=torch.int64, device=DEV)
    clock = P.T5DecodeClock(MAX_LEN, DEV)
    ld = c["qkv"].stride(0)
    stream = _lib.stream_of(out)

    def attn(live_ptr, clock_ptr, **over):
        a = _lib.T5DecodeAttnArgs(
            q=q.data_ptr(), ldq=ld, k_new=kn.data_ptr(), ldk=ld, v_new=vn.data_ptr(), ldv=ld, k=cache.k.data_ptr(),
            v=cache.v.data_ptr(), bias_by_distance=c["table"].data_ptr(), key_mask=None, out=out.data_ptr(), B=B,
            n_heads=NH, d_kv=d, max_len=MAX_LEN, t=0, dtype=_lib.BF16, mode=_lib.T5_ATTN_SELF)
        for k, v in over.items():
            setattr(a, k, v)
        return _lib.query("trlx_t5_decode_attn_live", ctypes.byref(a), live_ptr, clock_ptr, stream)

    lp, cp = live.data_ptr(), clock.record.data_ptr()
    cross = dict(mode=_lib.T5_ATTN_CROSS, k_new=None, v_new=None, bias_by_distance=None, k=k_enc.data_ptr(),
                 v=v_enc.data_ptr(), max_len=8)
    assert attn(None, None) == C.ERR_ARG and attn(lp + 4, None) == C.ERR_ARG and attn(lp, cp + 4) == C.ERR_ARG
    assert attn(lp, cp, **cross) == C.ERR_ARG                     # a clock with the cross mode
    for over in (dict(d_kv=32), dict(dtype=_lib.I64), dict(q=None), dict(k_new=None), dict(ldq=inner - 8),
                 dict(out=out.data_ptr() + 2), dict(max_len=0), dict(t=MAX_LEN), dict(t=-1)):
        assert attn(lp, None, **over) == C.ERR_ARG, over          # what the host-t entry refuses
    assert _lib.query("trlx_t5_decode_attn_live", None, lp, None, stream) == C.ERR_ARG
    torch.cuda.synchronize()
    assert C.same(out, torch.full_like(out, C.GUARD)) and C.same(cache.k, torch.full_like(cache.k, C.GUARD))
    assert attn(lp, cp, t=MAX_LEN + 3) == 0 and attn(lp + 8, None) == 0 and attn(lp, None, **cross) == 0
    torch.cuda.synchronize()
    assert not C.same(out, torch.full_like(out, C.GUARD))
