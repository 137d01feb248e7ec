"""The grouped decode cross-attention on MFMA at d_kv 256 without a GPU: the header's declarations,
the bindings and the package exports, every refusal of trlx_t5_decode_attn_group_d256 (each returns
before any launch, so aligned dummy addresses stand for device memory), the host functions against
their formulas and the wrapper's routes off the device."""
import ctypes
import inspect
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_cross_split_checks as S
import t5_rollout_checks as C
from test_t5_cross_group_cpu import HEADER, BASE, group_args

WS = BASE + (6 << 24)
NAMES = ("t5_decode_cross_attention_grouped_mma_d256", "t5_decode_cross_attention_grouped_mma_d256_geometry",
         "t5_decode_cross_attention_grouped_mma_d256_plan", "t5_decode_cross_attention_grouped_mma_d256_workspace_bytes")


def test_the_header_the_bindings_and_the_package_name_the_entries():
    flat = re.sub(r"\s+", " ", HEADER)
    for decl in ("int trlx_t5_decode_attn_group_d256(const TrlxT5DecodeAttnGroupArgs* a, int64_t splits, void* workspace, "
                 "int64_t workspace_bytes, void* stream);",
                 "int64_t trlx_t5_decode_attn_group_d256_workspace_bytes(int64_t rows, int64_t n_heads, int64_t S, "
                 "int64_t splits);",
                 "int trlx_t5_decode_attn_group_d256_geometry(int64_t S, int64_t splits, TrlxT5DecodeAttnGroupD256Geometry* g);",
                 "int trlx_t5_decode_attn_group_d256_plan(int64_t P, int64_t G, int64_t n_heads, int64_t S);"):
        assert decl in flat, decl
    body = re.search(r"typedef struct TrlxT5DecodeAttnGroupD256Geometry \{(.*?)\} TrlxT5DecodeAttnGroupD256Geometry;",
                     HEADER, re.S).group(1)
    names = re.findall(r"int64_t (\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _lib.T5DecodeAttnGroupD256Geometry._fields_]
    assert all(t is ctypes.c_int64 for _, t in _lib.T5DecodeAttnGroupD256Geometry._fields_)
    sig, i64, vp = _lib.SIGNATURES, ctypes.c_int64, ctypes.c_void_p
    assert sig["trlx_t5_decode_attn_group_d256"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeAttnGroupArgs), i64, vp, i64, vp])
    assert sig["trlx_t5_decode_attn_group_d256_workspace_bytes"] == (i64, [i64] * 4)
    assert sig["trlx_t5_decode_attn_group_d256_geometry"] == (ctypes.c_int, [i64, i64, ctypes.POINTER(_lib.T5DecodeAttnGroupD256Geometry)])
    assert sig["trlx_t5_decode_attn_group_d256_plan"] == (ctypes.c_int, [i64] * 4)
    for name in NAMES:
        assert name in P.__all__ and getattr(P, name) is getattr(P.t5_decode, name)
    assert list(inspect.signature(P.t5_decode_cross_attention_grouped_mma_d256).parameters) == [
        "q", "k_enc", "v_enc", "key_mask", "live", "n_heads", "splits", "workspace"]
    assert inspect.signature(P.t5_decode_cross_attention_grouped_mma) == inspect.signature(P.t5_decode_cross_attention_grouped)


def d256_args(**over):
    """The legal call of group_args at d_kv 256: P 3, G 4, nH 5, S 9, bf16, contiguous [P, nH, S, d]."""
    nH, d, Sn = 5, 256, 9
    f = dict(ldq=nH * d, k_stride_p=nH * Sn * d, k_stride_h=Sn * d, k_stride_s=d, v_stride_p=nH * Sn * d,
             v_stride_h=Sn * d, v_stride_s=d, d_kv=d)
    f.update(over)
    return group_args(**f)


NEED = 12 * 5 * 1 * 258 * 4    # the legal call: 9 keys are one block, so one range at any split
REFUSED = [
    ("d_kv 64", dict(d_kv=64), {}), ("d_kv 128", dict(d_kv=128), {}), ("fp32", dict(dtype=_lib.F32), {}),
    ("splits 0", {}, dict(splits=0)), ("splits 9", {}, dict(splits=9)),
    ("a NULL workspace", {}, dict(ws=None)), ("a misaligned workspace", {}, dict(ws=WS + 8)),
    ("a workspace one byte short", {}, dict(nbytes=NEED - 1)),
    ("NULL q", dict(q=None), {}), ("NULL k", dict(k=None), {}), ("NULL v", dict(v=None), {}), ("NULL out", dict(out=None), {}),
    ("a key stride not whole vectors", dict(k_stride_s=256 + 12), {}), ("ldq not whole vectors", dict(ldq=5 * 256 + 4), {}),
    ("too many query tiles", dict(P=1, G=1 << 21), {}),
]


@pytest.mark.parametrize("name,over,call", REFUSED, ids=[n for n, _, _ in REFUSED])
def test_every_refusal_comes_before_any_launch(name, over, call):
    f = dict(splits=2, ws=WS, nbytes=NEED)
    f.update(call)
    a = d256_args(**over)
    assert _lib.query("trlx_t5_decode_attn_group_d256", ctypes.byref(a), f["splits"], f["ws"], f["nbytes"], None) == C.ERR_ARG, name
    assert _lib.query("trlx_last_error").decode().startswith("t5 grouped d256 decode attention")
    assert _lib.query("trlx_t5_decode_attn_group_d256", None, 2, WS, NEED, None) == C.ERR_ARG


def test_geometry_workspace_and_plan_follow_their_formulas():
    geometry, nbytes = P.t5_decode_cross_attention_grouped_mma_d256_geometry, P.t5_decode_cross_attention_grouped_mma_d256_workspace_bytes
    for Sn in (1, 32, 33, 512, 2048):
        nblk = -(-Sn // 32)
        for X in (1, 3, 8):
            g = geometry(Sn, X)
            cb = -(-nblk // X)
            assert g == dict(waves=4, block_keys=32, tile=16, cb=cb, ranges=-(-nblk // cb), max_splits=8), (Sn, X, g)
            assert 1 <= g["ranges"] <= X
            owner = [[x for x in range(g["ranges"]) if x * cb <= j // 32 < min(nblk, (x + 1) * cb)] for j in range(Sn)]
            assert all(len(o) == 1 for o in owner) and owner[-1] == [g["ranges"] - 1]   # every key in one range, none empty
            for rows, nH in ((1, 1), (12, 5), (128, 16)):
                assert nbytes(rows, nH, Sn, X) == (0 if X == 1 else rows * nH * g["ranges"] * 258 * 4)
        for Pn, Gn, nH in ((128, 1, 16), (8, 16, 16), (2, 64, 16), (1, 8, 16), (3, 17, 5)):
            x = P.t5_decode_cross_attention_grouped_mma_d256_plan(Pn, Gn, nH, Sn)
            assert 1 <= x <= 8 and x == P.t5_decode_cross_attention_grouped_mma_d256_plan(Pn, Gn, nH, Sn)
    for bad in ((0, 1), (-1, 1), (9, 0), (9, 9)):
        with pytest.raises(ValueError, match="grouped d256 decode attention geometry"):
            geometry(*bad)
    assert nbytes(0, 5, 9, 2) == nbytes(12, 0, 9, 2) == nbytes(12, 5, 0, 2) == nbytes(12, 5, 9, 9) == 0
    assert P.t5_decode_cross_attention_grouped_mma_d256_plan(0, 1, 16, 512) == 1


def test_off_the_device_and_for_fp16_the_call_is_the_grouped_mma_call():
    c = S.group_case(torch.bfloat16, 256, 9, "right", 4)
    h = {k: c[k].to(torch.float16) for k in ("q", "K", "V")}          # a dtype no kernel takes: torch's route
    want = P.t5_decode_cross_attention_grouped_mma(h["q"], h["K"], h["V"], c["mask"])
    for X in (None, 1, 3):
        assert C.same(P.t5_decode_cross_attention_grouped_mma_d256(h["q"], h["K"], h["V"], c["mask"], splits=X), want)
    with pytest.raises(ValueError) as mine:                          # bf16 on the CPU: there is no CPU path
        P.t5_decode_cross_attention_grouped_mma_d256(c["q"], c["K"], c["V"], c["mask"])
    with pytest.raises(ValueError) as theirs:
        P.t5_decode_cross_attention_grouped_mma(c["q"], c["K"], c["V"], c["mask"])
    assert str(mine.value) == str(theirs.value)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="splits"):
            P.t5_decode_cross_attention_grouped_mma_d256(c["q"], c["K"], c["V"], splits=bad)
