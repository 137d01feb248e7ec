"""The fp8 encoder keys / values on the CPU: the torch fallback of t5_quantize_cross_kv (the
restatement the kernel is held to, bit for bit, by tests/test_gpu_t5_cross_kv8.py) against the
quantiser written from its definition (t5_cross_kv8_checks.ref_quantize), the scale rule at its
edges, ties and subnormals, dequantize(), masked rows, and the binding."""
import ctypes
import os
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_decode_attn_checks as A
import t5_cross_kv8_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quantize(K, V, mask=None, **kw):
    return P.t5_quantize_cross_kv(K, V, mask, **kw)


@pytest.mark.parametrize("kind", A.MASKS)
@pytest.mark.parametrize("d", C.D_KVS)
def test_fallback_is_torchs_cast_of_the_exactly_scaled_values(d, kind):
    for S in C.QUANT_S:
        c = A.cross_case(torch.bfloat16, d, S, kind)
        K, V = A.poison(c["K"], c["mask"]), A.poison(c["V"], c["mask"])
        want = C.ref_quantize(K, c["mask"]) + C.ref_quantize(V, c["mask"])
        for name, (k_in, nh) in C.layouts(K).items():
            v_in = C.layouts(V)[name][0]
            got = quantize(k_in, v_in, c["mask"], n_heads=nh)
            assert got.k8.dtype == torch.float8_e4m3fn and got.k8.shape == (C.B, C.NH, S, d) and got.k8.is_contiguous()
            assert got.k_scale.dtype == torch.float32 and got.k_scale.shape == (C.B, C.NH)
            assert C.quantised_equal(got, *want), (S, name)


def test_scale_rule_at_its_edges():
    n, S, d = len(C.EDGES), 3, 64
    K = torch.zeros(1, n, S, d)
    for h, (_, amax, _) in enumerate(C.EDGES):
        K[0, h, 1, 5] = -amax                   # the sign does not matter
        K[0, h, 2, 7] = amax / 3
    K = K.to(torch.bfloat16)
    assert [float(K[0, h, 1, 5]) for h in range(n)] == [-a for _, a, _ in C.EDGES], "the edges are bf16 values"
    got = quantize(K, K)
    for h, (name, amax, e) in enumerate(C.EDGES):
        assert C.exponent(amax) == e, name
        assert float(got.k_scale[0, h]) == 2.0 ** e and float(got.v_scale[0, h]) == 2.0 ** e, name
        if amax and e not in (C.E_MIN, C.E_MAX):
            assert amax * 2.0 ** -e <= 448.0 < amax * 2.0 ** -(e - 1), name
    assert C.quantised_equal(got, *(C.ref_quantize(K) * 2))


def test_ties_and_subnormals_with_scale_one():
    d = 64
    K = torch.zeros(1, 1, 2, d)
    K[0, 0, 0, :len(C.TIES)] = torch.tensor([v for v, _ in C.TIES])
    K[0, 0, 1, :len(C.TIES)] = -torch.tensor([v for v, _ in C.TIES])
    K[0, 0, 0, d - 1] = 448.0
    K = K.to(torch.bfloat16)
    got = quantize(K, K)
    assert float(got.k_scale) == 1.0
    kept = got.k8.float()
    want = torch.tensor([w for _, w in C.TIES])
    assert torch.equal(kept[0, 0, 0, :len(C.TIES)], want) and torch.equal(kept[0, 0, 1, :len(C.TIES)], -want)
    assert torch.equal(got.k8.view(torch.uint8), K.float().to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("d", C.D_KVS)
def test_dequantize_is_exact_in_bf16(d):
    c = C.special_case(d)
    got = quantize(c["K"], c["V"], c["mask"])
    for x8, s, deq in zip((got.k8, got.v8), (got.k_scale, got.v_scale), got.dequantize()):
        exact = x8.float().double() * s.double()[:, :, None, None]
        assert deq.dtype == torch.bfloat16 and deq.shape == x8.shape
        finite = torch.isfinite(exact)       # the upper clamp pushes bf16's largest values to the NaN byte
        assert finite.float().mean() > 0.99
        assert torch.equal(deq.double()[finite], exact[finite]) and torch.isnan(deq.double()[~finite]).all()


@pytest.mark.parametrize("d", C.D_KVS)
def test_masked_rows_are_zero_bytes_and_stay_out_of_amax(d):
    c = C.special_case(d)
    mask = c["mask"]
    got = quantize(c["K"], c["V"], mask)
    assert C.quantised_equal(got, *(C.ref_quantize(c["K"], mask) + C.ref_quantize(c["V"], mask)))
    dead = (mask == 0)[:, None, :, None].expand_as(got.k8)
    assert not got.k8.view(torch.uint8)[dead].any() and not got.v8.view(torch.uint8)[dead].any()
    assert torch.equal(got.k_scale[1], torch.ones(C.NH)) and torch.equal(got.v_scale[1], torch.ones(C.NH))   # fully masked
    assert torch.equal(got.k_scale[:, 1], torch.ones(C.B))                                                   # all zero
    # a huge value in a masked row changes nothing
    K2 = c["K"].clone()
    K2[2, :, 1] = 3.0e38
    assert C.quantised_equal(quantize(K2, c["V"], mask), *(C.ref_quantize(c["K"], mask) + C.ref_quantize(c["V"], mask)))


def test_a_live_non_finite_element_poisons_its_block_only():
    c = A.cross_case(torch.bfloat16, 64, 9, "holes")
    K, V = c["K"].clone(), c["V"].clone()
    live_row = int(torch.nonzero(c["mask"][1])[0])
    K[1, 2, live_row, 3] = float("inf")
    V[0, 4, int(torch.nonzero(c["mask"][0])[0]), 0] = float("nan")
    got = quantize(K, V, c["mask"])
    assert C.quantised_equal(got, *(C.ref_quantize(K, c["mask"]) + C.ref_quantize(V, c["mask"])))
    bad_k, bad_v = torch.isnan(got.k_scale), torch.isnan(got.v_scale)
    assert bad_k.sum() == 1 and bad_k[1, 2] and bad_v.sum() == 1 and bad_v[0, 4]
    on = (c["mask"] != 0)
    assert (got.k8.view(torch.uint8)[1, 2][on[1]] == 0x7f).all() and not got.k8.view(torch.uint8)[1, 2][~on[1]].any()


def test_out_argument_and_cpu_attention_fallback():
    c = A.cross_case(torch.bfloat16, 64, 33, "left")
    pre = P.T5CrossKV8(C.B, C.NH, 33, 64, "cpu")
    got = quantize(c["K"], c["V"], c["mask"], out=pre)
    assert got is pre and C.quantised_equal(pre, *(C.ref_quantize(c["K"], c["mask"]) + C.ref_quantize(c["V"], c["mask"])))
    k, v = pre.dequantize()
    want = P.t5_decode._torch_cross_attention(c["q"], k, v, c["mask"])
    assert torch.equal(P.t5_decode_cross_attention_kv8(c["q"], pre, c["mask"]), want)
    live = torch.tensor([1, 0, 5])
    out = P.t5_decode_cross_attention_kv8(c["q"], pre, c["mask"], live=live)
    assert torch.equal(out[0], want[0]) and torch.equal(out[2], want[2]) and not out[1].any()
    with pytest.raises(ValueError):
        quantize(c["K"], c["V"], c["mask"], out=P.T5CrossKV8(C.B, C.NH, 32, 64, "cpu"))
    with pytest.raises(ValueError):
        quantize(c["K"].float(), c["V"].float())
    with pytest.raises(ValueError):
        quantize(c["K"].reshape(C.B, 33 * C.NH, 64), c["V"].reshape(C.B, 33 * C.NH, 64))     # 3-D without n_heads
    with pytest.raises(ValueError):
        quantize(c["K"], c["V"], c["mask"][:, :-1])
    with pytest.raises(TypeError):
        P.t5_decode_cross_attention_kv8(c["q"], (k, v))
    assert live.tolist() == [1, 0, 5]


def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    body = re.search(r"typedef struct TrlxT5CrossKvQuantArgs \{(.*?)\} TrlxT5CrossKvQuantArgs;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (x for x in body.split(";") if x.strip()):      # `type a, b, c` declares three fields
        first, *more = decl.split(",")
        fields += [re.findall(r"\w+", first)[-1]] + [m.strip() for m in more]
    assert fields == [f[0] for f in _lib.T5CrossKvQuantArgs._fields_]
    assert ctypes.sizeof(_lib.T5CrossKvQuantArgs) == 8 * len(fields)
    assert re.search(r"int trlx_t5_decode_attn_kv8\(const TrlxT5DecodeAttnArgs\* a, const float\* k_scale, "
                     r"const float\* v_scale,\s*const int64_t\* live, void\* stream\);", txt)
    assert _lib.SIGNATURES["trlx_t5_decode_attn_kv8"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeAttnArgs)] + [ctypes.c_void_p] * 4)
    assert _lib.SIGNATURES["trlx_t5_cross_kv_quantize"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5CrossKvQuantArgs), ctypes.c_void_p])
