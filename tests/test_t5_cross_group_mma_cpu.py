"""The grouped decode cross-attention on MFMA without a GPU: the header's declaration, the binding's
signature, the package export, refusals of trlx_t5_decode_attn_group_mma (each returns before any
launch, so aligned dummy addresses stand for device memory) and the wrapper's route off the device."""
import ctypes
import inspect
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_cross_group_checks as G
import t5_rollout_checks as C
from test_t5_cross_group_cpu import HEADER, BASE, group_args


def test_the_header_the_binding_and_the_package_name_the_entry():
    flat = re.sub(r"\s+", " ", HEADER)
    assert "int trlx_t5_decode_attn_group_mma(const TrlxT5DecodeAttnGroupArgs* a, void* stream);" in flat
    assert "int trlx_t5_decode_attn_group_mma_waves(int64_t d_kv);" in flat
    assert _lib.SIGNATURES["trlx_t5_decode_attn_group_mma"] == _lib.SIGNATURES["trlx_t5_decode_attn_group"]
    assert hasattr(_lib.load(), "trlx_t5_decode_attn_group_mma")
    assert "t5_decode_cross_attention_grouped_mma" in P.__all__
    assert P.t5_decode_cross_attention_grouped_mma is P.t5_decode.t5_decode_cross_attention_grouped_mma
    assert inspect.signature(P.t5_decode_cross_attention_grouped_mma) == inspect.signature(P.t5_decode_cross_attention_grouped)
    waves = [_lib.query("trlx_t5_decode_attn_group_mma_waves", d) for d in (64, 128, 32)]
    assert waves[0] in (4, 8, 16) and waves[1] in (4, 8, 16) and waves[2] == 0


REFUSED = [("fp32", dict(dtype=_lib.F32)), ("an int64 dtype", dict(dtype=_lib.I64)), ("d_kv 32", dict(d_kv=32)),
           ("NULL q", dict(q=None)), ("NULL k", dict(k=None)), ("NULL v", dict(v=None)), ("NULL out", dict(out=None)),
           ("G 0", dict(G=0)), ("a key stride not whole vectors", dict(k_stride_s=64 + 12)),
           ("a head stride below d_kv", dict(v_stride_h=56)), ("ldq not whole vectors", dict(ldq=5 * 64 + 4)),
           ("k off 16 bytes", dict(k=BASE + (1 << 24) + 2)), ("live off 8 bytes", dict(live=BASE + (4 << 24) + 4)),
           ("too many query tiles", dict(P=1, G=1 << 21))]


@pytest.mark.parametrize("name,over", REFUSED, ids=[n for n, _ in REFUSED])
def test_every_refusal_comes_before_any_launch(name, over):
    a = group_args(**over)
    assert _lib.query("trlx_t5_decode_attn_group_mma", ctypes.byref(a), None) == C.ERR_ARG, name
    assert "grouped mma decode attention" in _lib.query("trlx_last_error").decode()
    assert _lib.query("trlx_t5_decode_attn_group_mma", None, None) == C.ERR_ARG


def test_off_the_device_the_call_is_the_grouped_call():
    c = G.group_case(torch.bfloat16, 64, 9, "right", 4)
    h = {k: c[k].to(torch.float16) for k in ("q", "K", "V")}          # a dtype no kernel takes: torch's route
    assert C.same(P.t5_decode_cross_attention_grouped_mma(h["q"], h["K"], h["V"], c["mask"]),
                  P.t5_decode_cross_attention_grouped(h["q"], h["K"], h["V"], c["mask"]))
    with pytest.raises(ValueError) as mine:                          # bf16 on the CPU: there is no CPU path
        P.t5_decode_cross_attention_grouped_mma(c["q"], c["K"], c["V"], c["mask"])
    with pytest.raises(ValueError) as theirs:
        P.t5_decode_cross_attention_grouped(c["q"], c["K"], c["V"], c["mask"])
    assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError, match="whole multiple"):
        P.t5_decode_cross_attention_grouped_mma(c["q"][:-1], c["K"], c["V"])
