"""Host-side checks of the d_kv 256 attention backward (no GPU): trlx_t5_attention_bwd_tiles_d is
declared, bound and answers without a device, t5_attention_train.tiles mirrors it, and a CPU or
fp32 d 256 training call still runs the torch route under autograd."""
import ctypes
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C
import t5_attention_bwd_checks as CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TR = P.t5_attention_train


def test_bwd_tiles_d_is_declared_bound_and_answers_without_a_device():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    assert ("int trlx_t5_attention_bwd_tiles_d(int64_t d_kv, int* dq_q_tile, int* dq_kv_tile, int* dkv_k_tile, "
            "int* dkv_q_tile);") in txt
    res, args = _lib.SIGNATURES["trlx_t5_attention_bwd_tiles_d"]
    assert res is ctypes.c_int and args == [ctypes.c_int64] + [ctypes.POINTER(ctypes.c_int)] * 4
    for d in (64, 128, 256):
        t = [ctypes.c_int(0) for _ in range(4)]
        _lib.call("trlx_t5_attention_bwd_tiles_d", d, *[ctypes.byref(x) for x in t])
        assert tuple(x.value for x in t) == TR.tiles(d)
        _lib.call("trlx_t5_attention_bwd_tiles_d", d, None, ctypes.byref(t[0]), None, None)   # any pointer may be NULL
        assert t[0].value == TR.tiles(d)[1]
    assert TR.tiles(64) == TR.tiles(128) == (TR.DQ_Q_TILE, TR.DQ_KV_TILE, TR.DKV_K_TILE, TR.DKV_Q_TILE)
    for bad in (96, 0):
        with pytest.raises(ValueError, match="status 5"):
            _lib.call("trlx_t5_attention_bwd_tiles_d", bad, None, None, None, None)
    with pytest.raises(ValueError, match="d_kv 96"):
        TR.tiles(96)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cpu_and_fp32_d256_training_calls_run_the_torch_route(dtype):
    T = 9
    c = C.case(256, T, T, "holes", dtype=dtype)
    dout = CB.make_dout(256, T, T).to(dtype)
    table64 = CB.table_from(c["W"], T, T, True)
    want = CB.oracle_grads(c["q"], c["k"], c["v"], dout, table64, c["mask"])
    kz, vz = C.poison(c["k"], c["mask"], 0.0), C.poison(c["v"], c["mask"], 0.0)
    q, k, v = (x.clone().requires_grad_() for x in (c["q"], kz, vz))
    table = table64.float().requires_grad_()
    out = TR(q, k, v, bias=table, key_mask=c["mask"])
    assert out.grad_fn is not None and "T5AttentionFn" not in type(out.grad_fn).__name__
    g = torch.autograd.grad(out, [q, k, v, table], dout)
    got = dict(dq=g[0], dk=g[1], dv=g[2], dbias=g[3])
    yard = CB.eager_grads(c["q"], kz, vz, dout, table64.float(), c["mask"])
    for n, (e_k, e_t, lim) in CB.judge(got, yard, want).items():
        assert e_k <= (lim if dtype == torch.bfloat16 else 1e-4), (n, e_k, e_t, lim)
