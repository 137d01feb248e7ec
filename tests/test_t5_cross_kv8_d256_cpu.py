"""The fp8 encoder keys / values at d_kv 256 on the CPU: the torch fallback of the quantiser against
the quantiser written from its definition, the attention fallback against the torch expressions on
dequantize(), and the device-free geometry / workspace helpers of trlx_t5_decode_attn_kv8_d256."""
import pytest
import torch

import trlx_t5_amd as P
import t5_decode_attn_checks as A
import t5_cross_kv8_checks as C

D = 256


@pytest.mark.parametrize("kind", A.MASKS)
def test_fallbacks_at_256(kind):
    for S in C.QUANT_S:
        c = A.cross_case(torch.bfloat16, D, S, kind)
        K, V = A.poison(c["K"], c["mask"]), A.poison(c["V"], c["mask"])
        got = P.t5_quantize_cross_kv(K, V, c["mask"])
        assert got.k8.shape == (C.B, C.NH, S, D) and C.quantised_equal(got, *(C.ref_quantize(K, c["mask"]) + C.ref_quantize(V, c["mask"])))
        k, v = got.dequantize()
        want = P.t5_decode._torch_cross_attention(c["q"], k, v, c["mask"])
        for splits in (None, 1, 3):   # the CPU route ignores it
            assert torch.equal(P.t5_decode_cross_attention_kv8(c["q"], got, c["mask"], splits=splits), want)
    with pytest.raises(ValueError, match="splits"):
        P.t5_decode_cross_attention_kv8(c["q"], got, c["mask"], splits=17)


@pytest.mark.parametrize("splits", (1, 2, 3, 16))
@pytest.mark.parametrize("S", (1, 63, 64, 65, 512))
def test_geometry_and_workspace(S, splits):
    g = P.t5_decode_cross_attention_kv8_d256_geometry(S, splits)
    assert (g["rows_per_wave_load"], g["lane_groups"], g["keys_per_trip"], g["max_splits"]) == (4, 16, 64, 16)
    assert g["rows_per_wave_load"] * 16 == 64 and g["lane_groups"] * 4 == g["keys_per_trip"]   # 16 lanes a row, 4 in flight
    C_, R = g["keys_per_range"], g["ranges"]
    assert C_ % g["keys_per_trip"] == 0 and 1 <= R <= splits
    assert (R - 1) * C_ < S <= R * C_                      # the ranges cover S exactly once, none empty
    assert C_ == -(-(-(-S // 64)) // splits) * 64          # ceil(ceil(S / 64) / splits) whole trips
    for B, nH in ((1, 1), (3, 5), (128, 16)):
        assert P.t5_decode_cross_attention_kv8_d256_workspace_bytes(B, nH, splits) == splits * B * nH * 258 * 4
