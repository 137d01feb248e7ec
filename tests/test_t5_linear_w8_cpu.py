"""fp8 projection weights without a GPU: the torch route of t5_quantize_linear_weight against the
quantiser written from its definition, the CPU route of t5_decode_linear_w8, the default wave count
and the binding against the header."""
import ctypes
import os
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_cross_kv8_checks as C
import t5_decode_linear_checks as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,K", ((16, 64), (48, 320)))
def test_the_torch_quantiser_is_the_definition_bit_for_bit(N, K):
    w = torch.randn(3 * N, K, generator=torch.Generator().manual_seed(K))
    w[N], w[N + 1], w[N + 2] = 0.0, w[N + 1] * 1e30, w[N + 2] * 1e-30
    w[N + 3, :len(C.TIES)] = torch.tensor([v for v, _ in C.TIES])
    w[N + 3, K - 1] = 448.0
    w[N + 4, 1] = float("nan")
    w = w.to(torch.bfloat16)
    want8, want_scale = C.ref_quantize(w[N:2 * N][None, :, None, :])
    got = P.t5_quantize_linear_weight(w[N:2 * N])
    assert torch.equal(got.w8.view(torch.uint8), want8[0, :, 0]) and C.same_scales(got.scale, want_scale[0])
    assert got.dequantize().dtype == torch.bfloat16 and tuple(got.shape) == (N, K)
    with pytest.raises(ValueError):
        P.t5_quantize_linear_weight(w.float())


def test_the_cpu_route_is_t5_decode_linear_on_the_dequantised_weight():
    x, w, nw, _ = L.inputs(3, 16, 64, True, seed=4)
    w8 = P.t5_quantize_linear_weight(w)
    got = P.t5_decode_linear_w8(x, w8, norm_weight=nw, act="silu", gated=True)
    assert torch.equal(got, P.t5_decode_linear(x, w8.dequantize(), norm_weight=nw, act="silu", gated=True))
    with pytest.raises(ValueError, match="multiple of 64"):
        P.t5_decode_linear_w8(x[:, :32], P.T5LinearW8(w8.w8[:, :32].contiguous(), w8.scale))


def test_the_default_wave_count_is_a_function_of_n_k_and_gated_alone():
    geo = P.t5_linear_w8.linear_w8_geometry
    for N, K, gated in ((4096, 4096, False), (768, 768, False), (10240, 4096, True), (16, 64, False), (32128, 4096, False)):
        g = geo(N, K, gated)
        assert g == geo(N, K, gated) and g["waves"] in P.t5_linear_w8.W8_WAVES and g["turns"] == -(-K // 256)
        assert g["waves"] == 4 or g["waves"] <= g["turns"]              # no more waves than K has turns
    assert (g["k_per_chunk"], g["cols_per_block"], g["max_k"], g["norm_max_k"]) == (64, 16, 16384, 8192)


def test_the_binding_mirrors_the_header():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read(), flags=re.S)
    for c_name, mirror in (("trlx_t5_decode_linear_w8_args", _lib.T5DecodeLinearW8Args),
                           ("TrlxT5DecodeLinearW8Geometry", _lib.T5DecodeLinearW8Geometry)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), header, re.S).group(1)
        assert re.findall(r"(\w+);", body) == [n for n, _ in mirror._fields_]
    assert _lib.SIGNATURES["trlx_t5_decode_linear_w8"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeLinearW8Args), ctypes.c_void_p])
    for name in ("T5LinearW8", "t5_quantize_linear_weight", "t5_decode_linear_w8", "T5DecodeBlockWeights8"):
        assert name in P.__all__ and hasattr(P, name)
