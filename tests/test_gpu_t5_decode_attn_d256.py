"""The decode-step self- and cross-attention at d_kv 256 on the GPU (k_t5_decode_attn<., 256, ...>:
32 lanes a bf16 key row, a whole wave an fp32 one) against the float64 oracle of
tests/t5_decode_attn_checks.py under that file's rule; t=clock against the host-t call bit for bit;
live= gives zeros for dead rows and the same bits for live ones.  B 3, nH 2, max_len 9, S 70."""
import pytest
import torch

import trlx_t5_amd as P
import t5_decode_attn_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, NH, D, MAX_LEN, S = 3, 2, 256, 9, 70


def rand(g, *shape, scale=1.0, dtype):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("what", ["self_t0", "self_t4", "self_t8", "cross_right", "cross_holes"])
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.dtype_name)
def test_decode_attention_d256(dtype, what):
    g = torch.Generator().manual_seed(256 + len(what) + (7 if dtype == torch.float32 else 0))
    s = D ** -0.25
    live = torch.tensor([1, 0, 1], dtype=torch.int64, device=DEV)
    if what.startswith("self"):
        t = int(what[6:])
        Q, K = (rand(g, B, NH, MAX_LEN, D, scale=s, dtype=dtype) for _ in range(2))
        V = rand(g, B, NH, MAX_LEN, D, dtype=dtype)
        W = torch.randn(C.NUM_BUCKETS, NH, generator=g)
        K64, V64 = K.double().clone(), V.double().clone()
        want = C.oracle_self_step(Q[:, :, t], K[:, :, t], V[:, :, t], K64, V64, t, W)
        table = P.t5_relative_bias_table(W.to(DEV), MAX_LEN)
        q, kn, vn = (x[:, :, t].contiguous().to(DEV) for x in (Q, K, V))

        def cache():   # columns below t filled, column t and above zeros
            ch = P.T5DecodeKVCache(B, NH, D, MAX_LEN, dtype, DEV)
            ch.k[:, :, :t] = K[:, :, :t].to(DEV)
            ch.v[:, :, :t] = V[:, :, :t].to(DEV)
            return ch

        c0, c1, c2 = cache(), cache(), cache()
        got = P.t5_decode_self_attention(q, kn, vn, c0, t, table)
        assert torch.equal(c0.k[:, :, t], kn) and torch.equal(c0.v[:, :, t], vn)
        assert float(c0.k[:, :, t + 1:].float().abs().max() if t + 1 < MAX_LEN else 0.0) == 0.0
        eager = C.eager_self(q, c0.k, c0.v, t, table)
        clock = P.T5DecodeClock(MAX_LEN, DEV)
        for _ in range(t):
            clock.advance()
        by_clock = P.t5_decode_self_attention(q, kn, vn, c1, clock, table)
        assert torch.equal(by_clock, got) and torch.equal(c1.k, c0.k) and torch.equal(c1.v, c0.v)
        lv = P.t5_decode_self_attention(q, kn, vn, c2, t, table, live=live)
        assert float(c2.k[1, :, t].float().abs().max()) == 0.0   # the dead row's column stays unwritten
    else:
        q = rand(g, B, NH, D, scale=s, dtype=dtype)
        K, V = rand(g, B, NH, S, D, scale=s, dtype=dtype), rand(g, B, NH, S, D, dtype=dtype)
        mask = C.make_mask(what[6:], B, S, g)
        want = C.oracle_cross(q, K, V, mask)
        q, mk = q.to(DEV), mask.to(DEV)
        kp, vp = C.poison(K, mask).to(DEV), C.poison(V, mask).to(DEV)
        got = P.t5_decode_cross_attention(q, kp, vp, mk)
        dead = (mask == 0)[:, None, :, None]
        eager = C.eager_cross(q, K.masked_fill(dead, 0).to(DEV), V.masked_fill(dead, 0).to(DEV), mk)
        lv = P.t5_decode_cross_attention(q, kp, vp, mk, live=live)
    assert tuple(got.shape) == (B, NH * D) and got.dtype == dtype and torch.isfinite(got).all()
    e_k, e_t = C.max_err(got, want), C.max_err(eager, want)
    lim = C.bound(dtype, e_t, want)
    print(dict(what=what, dtype=C.dtype_name(dtype), e_torch=e_t, e_kernel=e_k, bound=lim))
    assert e_k <= lim
    assert float(lv[1].float().abs().max()) == 0.0
    assert torch.equal(lv[0], got[0]) and torch.equal(lv[2], got[2])
