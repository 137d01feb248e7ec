"""The fp8 encoder keys / values on the GPU: trlx_t5_cross_kv_quantize against the CPU restatement
(the package's torch fallback, itself held to the definition by tests/test_t5_cross_kv8_cpu.py), bit
for bit, and trlx_t5_decode_attn_kv8 against the float64 oracle on the DEQUANTISED keys and values.

The attention rule is the bf16 kernel's, unchanged (t5_decode_attn_checks.bound):
    max|kernel - oracle| <= max|eager - oracle| + one bf16 ulp of max|oracle|
with eager = torch's own route on the device, fed the dequantised bf16 tensors.  byte * scale is
exact in bf16, so the kernel, the oracle and the eager route all start from the same values and no
constant for the quantisation enters.

Geometry of k_t5_decode_attn_kv8 (16 bytes = 16 elements a lane, 4 columns in flight per group):
    d_kv  64:  4 lanes a row, 16 rows a wave-wide load, 64 groups, 256 columns a trip
    d_kv 128:  8 lanes a row,  8 rows a wave-wide load, 32 groups, 128 columns a trip
ATTN_S holds both sides of each of those for both d_kv, and the S of the bf16 tests."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_decode_attn_checks as A
import t5_cross_kv8_checks as C
from t5_rollout_checks import ERR_ARG, GUARD, same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
WAVE_LOAD = {64: 16, 128: 8}
GROUPS = {64: 64, 128: 32}
TRIP = {64: 256, 128: 128}
ATTN_S = tuple(sorted(set(A.CROSS_S) | {e + o for g in (WAVE_LOAD, GROUPS, TRIP) for e in g.values() for o in (-1, 0, 1)}))
_ATTN = {}


def dev(x):
    return None if x is None else x.to(DEV)


def attn_case(d, S, kind):
    """cross_case quantised on the device (once per case), with the oracle and the eager error."""
    key = (d, S, kind)
    if key not in _ATTN:
        c = A.cross_case(BF, d, S, kind)
        kv8 = P.t5_quantize_cross_kv(dev(c["K"]), dev(c["V"]), dev(c["mask"]))
        Kd, Vd = kv8.dequantize()
        ref = A.oracle_cross(c["q"], Kd.cpu(), Vd.cpu(), c["mask"])
        eager = A.eager_cross(dev(c["q"]), Kd, Vd, dev(c["mask"]))
        assert torch.isfinite(eager.float()).all()
        _ATTN[key] = dict(q=dev(c["q"]), mask=dev(c["mask"]), kv8=kv8, ref=ref, e_torch=A.max_err(eager, ref), cpu=c)
    return _ATTN[key]


# ------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("kind", A.MASKS)
@pytest.mark.parametrize("d", C.D_KVS)
def test_quantiser_equals_the_cpu_restatement(d, kind):
    for S in C.QUANT_S:
        c = A.cross_case(BF, d, S, kind)
        K, V = A.poison(c["K"], c["mask"]), A.poison(c["V"], c["mask"])   # masked rows are not read
        want = P.t5_quantize_cross_kv(K, V, c["mask"])
        for name, (k_in, nh) in C.layouts(K).items():
            v_in = C.layouts(V)[name][0]
            k_dev, v_dev = dev(k_in), dev(v_in)
            assert k_dev.stride() == k_in.stride()
            got = P.t5_quantize_cross_kv(k_dev, v_dev, dev(c["mask"]), n_heads=nh)
            assert got.k8.is_cuda and got.k8.dtype == torch.float8_e4m3fn
            assert C.quantised_equal(got, want.k8.view(torch.uint8), want.k_scale, want.v8.view(torch.uint8), want.v_scale), (S, name)


@pytest.mark.parametrize("d", C.D_KVS)
def test_quantiser_ties_subnormals_zero_head_clamps_and_a_masked_row(d):
    c = C.special_case(d)
    want = P.t5_quantize_cross_kv(c["K"], c["V"], c["mask"])
    pre = P.T5CrossKV8(C.B, C.NH, c["K"].shape[2], d, DEV)
    pre.k8.view(torch.uint8).fill_(0x55)
    got = P.t5_quantize_cross_kv(dev(c["K"]), dev(c["V"]), dev(c["mask"]), out=pre)
    assert got is pre
    assert C.quantised_equal(got, want.k8.view(torch.uint8), want.k_scale, want.v8.view(torch.uint8), want.v_scale)
    assert float(got.k_scale[0, 0]) == 1.0 and not got.k8.view(torch.uint8)[1].any()
    kept = got.k8[0, 0, 0, :len(C.TIES)].float().cpu()
    assert torch.equal(kept, torch.tensor([w for _, w in C.TIES]))


def test_quantiser_non_finite_block_gives_nan_for_that_row_and_head_only():
    d, S = 64, 33
    c = A.cross_case(BF, d, S, "holes")
    K, V = c["K"].clone(), c["V"].clone()
    K[1, 2, int(torch.nonzero(c["mask"][1])[0]), 3] = float("inf")
    V[0, 4, int(torch.nonzero(c["mask"][0])[-1]), 0] = float("nan")
    want = P.t5_quantize_cross_kv(K, V, c["mask"])
    got = P.t5_quantize_cross_kv(dev(K), dev(V), dev(c["mask"]))
    assert C.quantised_equal(got, want.k8.view(torch.uint8), want.k_scale, want.v8.view(torch.uint8), want.v_scale)
    out = P.t5_decode_cross_attention_kv8(dev(c["q"]), got, dev(c["mask"])).view(C.B, C.NH, d).float().cpu()
    nan = torch.isnan(out).all(dim=2)
    assert nan[1, 2] and nan[0, 4] and nan.sum() == 2 and torch.isfinite(out[~nan]).all()


def test_quantiser_refusals():
    d, S = 64, 9
    c = A.cross_case(BF, d, S, "right")
    K, V, mask = dev(c["K"]), dev(c["V"]), dev(c["mask"])
    kv8 = P.T5CrossKV8(C.B, C.NH, S, d, DEV)
    kv8.k8.view(torch.uint8).fill_(0x55)
    kv8.k_scale.fill_(GUARD)
    stream = _lib.stream_of(K)

    def quant(**over):
        a = _lib.T5CrossKvQuantArgs(
            k=K.data_ptr(), k_stride_b=K.stride(0), k_stride_h=K.stride(1), k_stride_s=K.stride(2),
            v=V.data_ptr(), v_stride_b=V.stride(0), v_stride_h=V.stride(1), v_stride_s=V.stride(2),
            key_mask=mask.data_ptr(), k8=kv8.k8.data_ptr(), v8=kv8.v8.data_ptr(), k_scale=kv8.k_scale.data_ptr(),
            v_scale=kv8.v_scale.data_ptr(), B=C.B, n_heads=C.NH, S=S, d_kv=d)
        for k, v in over.items():
            setattr(a, k, v)
        return _lib.query("trlx_t5_cross_kv_quantize", ctypes.byref(a), stream)

    for over in (dict(k=None), dict(v=None), dict(k8=None), dict(v8=None), dict(k_scale=None), dict(v_scale=None),
                 dict(d_kv=32), dict(B=0), dict(n_heads=0), dict(S=0), dict(k=K.data_ptr() + 2), dict(v8=kv8.v8.data_ptr() + 8),
                 dict(k_scale=kv8.k_scale.data_ptr() + 2), dict(key_mask=mask.data_ptr() + 4), dict(k_stride_s=d + 4),
                 dict(v_stride_h=-8), dict(k_stride_s=d - 8), dict(v_stride_h=d - 8)):
        assert quant(**over) == ERR_ARG, over
    assert _lib.query("trlx_t5_cross_kv_quantize", None, stream) == ERR_ARG
    torch.cuda.synchronize()
    assert (kv8.k8.view(torch.uint8) == 0x55).all() and (kv8.k_scale == GUARD).all()
    assert quant() == 0 and quant(key_mask=None) == 0
    with pytest.raises(ValueError):
        P.t5_quantize_cross_kv(K.float(), V.float())
    with pytest.raises(ValueError):
        P.t5_quantize_cross_kv(K, V, mask.to(torch.int32))


# ------------------------------------------------------------------ the attention
@pytest.mark.parametrize("kind", A.MASKS)
@pytest.mark.parametrize("d", C.D_KVS)
def test_attention_against_the_oracle_on_the_dequantised_values(d, kind):
    for S in ATTN_S:
        c = attn_case(d, S, kind)
        out = P.t5_decode_cross_attention_kv8(c["q"], c["kv8"], c["mask"])
        assert out.dtype == BF and out.shape == (C.B, C.NH * d)
        e_kernel, limit = A.max_err(out, c["ref"]), A.bound(BF, c["e_torch"], c["ref"])
        print(f"kv8 d {d} S {S} {kind}: kernel {e_kernel:.3e} eager {c['e_torch']:.3e} bound {limit:.3e}")
        assert e_kernel <= limit, (S, e_kernel, limit)
        # the same values through the bf16 kernel: both are within the rule of one oracle
        Kd, Vd = c["kv8"].dequantize()
        assert A.max_err(P.t5_decode_cross_attention(c["q"], Kd, Vd, c["mask"]), c["ref"]) <= limit


@pytest.mark.parametrize("d", C.D_KVS)
def test_attention_repeats_and_does_not_depend_on_B_or_on_qs_stride(d):
    for S in (33, TRIP[d] + 1):
        c = attn_case(d, S, "holes")
        kv8, q, mask = c["kv8"], c["q"], c["mask"]
        out = P.t5_decode_cross_attention_kv8(q, kv8, mask)
        assert same(P.t5_decode_cross_attention_kv8(q, kv8, mask), out)
        inner = C.NH * d
        fused = torch.full((C.B, 3 * inner), float("nan"), dtype=BF, device=DEV)   # q as a slice of a qkv projection
        fused[:, inner:2 * inner] = q.reshape(C.B, inner)
        assert same(P.t5_decode_cross_attention_kv8(fused[:, inner:2 * inner], kv8, mask), out)
        assert same(P.t5_decode_cross_attention_kv8(q.reshape(C.B, C.NH, 1, d), kv8, mask), out)
        for b in range(C.B):                                                        # the same call at B = 1
            one = P.T5CrossKV8(1, C.NH, S, d, DEV)
            for dst, src in ((one.k8, kv8.k8), (one.v8, kv8.v8), (one.k_scale, kv8.k_scale), (one.v_scale, kv8.v_scale)):
                dst.copy_(src[b:b + 1])
            assert same(P.t5_decode_cross_attention_kv8(q[b:b + 1], one, mask[b:b + 1]), out[b:b + 1]), (S, b)


@pytest.mark.parametrize("d", C.D_KVS)
def test_a_fully_masked_row_gives_zeros(d):
    S = GROUPS[d] + 1
    c = A.cross_case(BF, d, S, "right")
    mask = c["mask"].clone()
    mask[1] = 0
    kv8 = P.t5_quantize_cross_kv(dev(A.poison(c["K"], mask)), dev(A.poison(c["V"], mask)), dev(mask))
    out = P.t5_decode_cross_attention_kv8(dev(c["q"]), kv8, dev(mask))
    assert not out[1].any() and out[0].any() and out[2].any() and torch.isfinite(out.float()).all()
    Kd, Vd = kv8.dequantize()
    ref = A.oracle_cross(c["q"], Kd.cpu(), Vd.cpu(), mask)
    e_torch = A.max_err(A.eager_cross(dev(c["q"]), Kd, Vd, dev(mask))[[0, 2]], ref[[0, 2]])
    assert A.max_err(out, ref) <= A.bound(BF, e_torch, ref)


# ------------------------------------------------------------------ live rows
@pytest.mark.parametrize("d", C.D_KVS)
def test_live_skips_dead_rows_and_keeps_live_rows(d):
    for S, kind in ((9, "none"), (GROUPS[d] + 1, "holes"), (TRIP[d] + 1, "left")):
        c = attn_case(d, S, kind)
        kv8, q, mask = c["kv8"], c["q"], c["mask"]
        want = P.t5_decode_cross_attention_kv8(q, kv8, mask)
        for pattern in ([1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 0, 7]):
            live = torch.tensor(pattern, dtype=torch.int64, device=DEV)
            on = live != 0
            bad = P.T5CrossKV8(C.B, C.NH, S, d, DEV)                # the dead rows' bytes and scales poisoned
            for dst, src in ((bad.k8, kv8.k8), (bad.v8, kv8.v8)):
                dst.view(torch.uint8).copy_(src.view(torch.uint8))
                dst.view(torch.uint8)[~on] = 0x7f
            for dst, src in ((bad.k_scale, kv8.k_scale), (bad.v_scale, kv8.v_scale)):
                dst.copy_(src)
                dst[~on] = float("nan")
            pq = q.clone()
            pq[~on] = float("nan")
            got = P.t5_decode_cross_attention_kv8(pq, bad, mask, live=live)
            assert same(got[on], want[on]), (S, pattern, "live rows")
            assert same(got[~on], torch.zeros_like(got[~on])), (S, pattern, "dead rows")
            assert live.tolist() == pattern


def test_one_captured_call_replays_with_live_rewritten():
    d, S = 64, TRIP[64] + 1
    c = attn_case(d, S, "holes")
    kv8, q, mask = c["kv8"], c["q"], c["mask"]
    live = torch.ones(C.B, dtype=torch.int64, device=DEV)
    patterns = ([1, 1, 1], [1, 0, 1], [0, 0, 3])
    want = [P.t5_decode_cross_attention_kv8(q, kv8, mask, live=torch.tensor(p, dtype=torch.int64, device=DEV)) for p in patterns]
    P.t5_decode_cross_attention_kv8(q, kv8, mask, live=live)        # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = P.t5_decode_cross_attention_kv8(q, kv8, mask, live=live)
    for p, w in zip(patterns, want):
        live.copy_(torch.tensor(p, dtype=torch.int64, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, w), p


# ------------------------------------------------------------------ refusals
def test_attention_refusals():
    d, S = 64, 9
    c = attn_case(d, S, "right")
    kv8, q, mask = c["kv8"], c["q"].reshape(C.B, C.NH * d), c["mask"]
    inner = C.NH * d
    out = torch.full((C.B, inner), GUARD, dtype=BF, device=DEV)
    live = torch.ones(C.B + 1, dtype=torch.int64, device=DEV)
    f32 = torch.zeros(16, dtype=torch.float32, device=DEV)
    stream = _lib.stream_of(out)
    ks, vs, lp = kv8.k_scale.data_ptr(), kv8.v_scale.data_ptr(), live.data_ptr()

    def attn(k_scale, v_scale, live_ptr, **over):
        a = _lib.T5DecodeAttnArgs(
            q=q.data_ptr(), ldq=inner, k_new=None, ldk=0, v_new=None, ldv=0, k=kv8.k8.data_ptr(), v=kv8.v8.data_ptr(),
            bias_by_distance=None, key_mask=mask.data_ptr(), out=out.data_ptr(), B=C.B, n_heads=C.NH, d_kv=d, max_len=S,
            t=0, dtype=_lib.BF16, mode=_lib.T5_ATTN_CROSS)
        for k, v in over.items():
            setattr(a, k, v)
        return _lib.query("trlx_t5_decode_attn_kv8", ctypes.byref(a), k_scale, v_scale, live_ptr, stream)

    # what the cross mode of trlx_t5_decode_attn refuses
    for over in (dict(d_kv=32), dict(dtype=_lib.I64), dict(q=None), dict(k=None), dict(v=None), dict(out=None),
                 dict(ldq=inner - 8), dict(ldq=inner + 4), dict(out=out.data_ptr() + 2), dict(q=q.data_ptr() + 2),
                 dict(max_len=0), dict(B=0), dict(n_heads=0), dict(k_new=q.data_ptr()), dict(v_new=q.data_ptr()),
                 dict(bias_by_distance=f32.data_ptr()), dict(key_mask=mask.data_ptr() + 4), dict(mode=7)):
        assert attn(ks, vs, None, **over) == ERR_ARG, over
    # its own
    assert attn(ks, vs, None, mode=_lib.T5_ATTN_SELF) == ERR_ARG
    assert attn(ks, vs, None, dtype=_lib.F32) == ERR_ARG
    assert attn(None, vs, None) == ERR_ARG and attn(ks, None, None) == ERR_ARG
    assert attn(ks + 2, vs, None) == ERR_ARG and attn(ks, vs + 2, None) == ERR_ARG
    assert attn(ks, vs, None, k=kv8.k8.data_ptr() + 8) == ERR_ARG and attn(ks, vs, None, v=kv8.v8.data_ptr() + 4) == ERR_ARG
    assert attn(ks, vs, lp + 4) == ERR_ARG
    assert _lib.query("trlx_t5_decode_attn_kv8", None, ks, vs, None, stream) == ERR_ARG
    torch.cuda.synchronize()
    assert same(out, torch.full_like(out, GUARD))
    assert attn(ks, vs, None) == 0 and attn(ks, vs, lp + 8) == 0 and attn(ks, vs, lp, key_mask=None) == 0
    torch.cuda.synchronize()
    assert same(out, P.t5_decode_cross_attention_kv8(q, kv8, None))
    # the Python entry
    with pytest.raises(ValueError):
        P.t5_decode_cross_attention_kv8(q.float(), kv8, mask)
    with pytest.raises(ValueError, match="live"):
        P.t5_decode_cross_attention_kv8(q, kv8, mask, live=live)
    with pytest.raises(ValueError, match="key_mask"):
        P.t5_decode_cross_attention_kv8(q, kv8, mask[:, :-1])
    with pytest.raises(TypeError):
        P.t5_decode_cross_attention_kv8(q, kv8.dequantize(), mask)
