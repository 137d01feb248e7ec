"""Host-side checks of the d_kv 256 attention (no GPU): the new entry is declared, bound and
exported, tiles() answers for the kernels' head sizes only, and a CPU or fp32 d 256 call still runs
the documented torch route, equal to the float64 oracle."""
import ctypes
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tiles_d_is_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    assert "int trlx_t5_attention_tiles_d(int64_t d_kv, int* q_tile, int* kv_tile);" in txt
    res, args = _lib.SIGNATURES["trlx_t5_attention_tiles_d"]
    assert res is ctypes.c_int and args == [ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    for d in (64, 128, 256):   # a host function: no device needed
        q_tile, kv_tile = ctypes.c_int(0), ctypes.c_int(0)
        _lib.call("trlx_t5_attention_tiles_d", d, ctypes.byref(q_tile), ctypes.byref(kv_tile))
        assert (q_tile.value, kv_tile.value) == P.t5_attention.tiles(d)
    with pytest.raises(ValueError, match="status 5"):
        _lib.call("trlx_t5_attention_tiles_d", 96, None, None)


def test_tiles_answers_for_the_kernels_only():
    q_tile, kv_tile = P.t5_attention.tiles(256)
    assert q_tile >= 32 and kv_tile >= 16
    assert P.t5_attention.tiles(64) == P.t5_attention.tiles(128) == (P.t5_attention.Q_TILE, P.t5_attention.KV_TILE)
    with pytest.raises(ValueError, match="d_kv 96"):
        P.t5_attention.tiles(96)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cpu_and_fp32_d256_calls_run_the_torch_route(dtype):
    c = C.case(256, 9, 9, "holes", dtype=dtype)
    table = P.t5_relative_bias_offsets(c["W"], 9, 9, True)
    want = C.oracle(c["q"], c["k"], c["v"], c["W"], True, mask=c["mask"])
    got = P.t5_attention(c["q"], C.poison(c["k"], c["mask"]), C.poison(c["v"], c["mask"]), bias=table, key_mask=c["mask"])
    assert got.dtype == dtype and tuple(got.shape) == (C.B, 9, C.NH * 256)
    if dtype == torch.bfloat16:   # torch's own bf16 rounding: the GPU test's rule against the eager route here
        kz, vz = C.poison(c["k"], c["mask"], 0.0), C.poison(c["v"], c["mask"], 0.0)
        assert C.max_err(got, want) <= C.bound(C.max_err(C.eager(c["q"], kz, vz, table, c["mask"]), want), want)
        return
    assert C.max_err(got, want) < 1e-5
    qg = c["q"].clone().requires_grad_()
    out = P.t5_attention_train(qg, c["k"], c["v"], bias=table, key_mask=c["mask"])   # d 256: torch under autograd
    out.sum().backward()
    assert torch.equal(out.detach(), P.t5_attention(c["q"], c["k"], c["v"], bias=table, key_mask=c["mask"]))
    assert qg.grad is not None and torch.isfinite(qg.grad).all()
