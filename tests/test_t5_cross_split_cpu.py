"""The split decode cross-attention without a GPU: the header's declarations, the ctypes mirror, the
host functions (geometry, workspace size, plan) and every refusal of trlx_t5_decode_attn_split (each
returns before any launch, so aligned dummy addresses stand for device memory), and the wrapper's
shape errors and its fall-back off the device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_cross_split_checks as S
import t5_rollout_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
BASE = 0x7f0000000000          # never dereferenced: every call below is refused before a launch
WS = BASE + (6 << 24)
CODES = {torch.bfloat16: _lib.BF16, torch.float32: _lib.F32}
GEOMETRIES = [(dt, d) for dt in (torch.bfloat16, torch.float32) for d in (64, 128)]


def test_the_header_declares_the_entries_and_keeps_the_abi_version():
    flat = re.sub(r"\s+", " ", HEADER)
    for decl in ("int trlx_t5_decode_attn_split(const TrlxT5DecodeAttnGroupArgs* a, int64_t splits, void* workspace, "
                 "int64_t workspace_bytes, void* stream);",
                 "int64_t trlx_t5_decode_attn_split_workspace_bytes(int64_t rows, int64_t n_heads, int64_t d_kv, "
                 "int64_t splits);",
                 "int trlx_t5_decode_attn_split_geometry(int dtype, int64_t d_kv, int64_t S, int64_t splits, "
                 "TrlxT5DecodeAttnSplitGeometry* g);",
                 "int trlx_t5_decode_attn_split_plan(int dtype, int64_t P, int64_t G, int64_t n_heads, int64_t d_kv, "
                 "int64_t S);"):
        assert decl in flat, decl
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", HEADER) and _lib.ABI_VERSION == 2
    body = re.search(r"typedef struct TrlxT5DecodeAttnSplitGeometry \{(.*?)\} TrlxT5DecodeAttnSplitGeometry;", HEADER, re.S).group(1)
    names = re.findall(r"int64_t (\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _lib.T5DecodeAttnSplitGeometry._fields_] == ["NG", "C", "ranges", "tile", "max_splits"]
    assert all(t is ctypes.c_int64 for _, t in _lib.T5DecodeAttnSplitGeometry._fields_)


def test_the_binding_lists_the_symbols_and_the_package_exports_the_wrappers():
    sig, i64, vp = _lib.SIGNATURES, ctypes.c_int64, ctypes.c_void_p
    assert sig["trlx_t5_decode_attn_split"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeAttnGroupArgs), i64, vp, i64, vp])
    assert sig["trlx_t5_decode_attn_split_workspace_bytes"] == (i64, [i64] * 4)
    assert sig["trlx_t5_decode_attn_split_geometry"] == (ctypes.c_int, [ctypes.c_int, i64, i64, i64,
                                                                        ctypes.POINTER(_lib.T5DecodeAttnSplitGeometry)])
    assert sig["trlx_t5_decode_attn_split_plan"] == (ctypes.c_int, [ctypes.c_int] + [i64] * 5)
    lib = _lib.load()
    for name in ("trlx_t5_decode_attn_split", "trlx_t5_decode_attn_split_workspace_bytes",
                 "trlx_t5_decode_attn_split_geometry", "trlx_t5_decode_attn_split_plan"):
        assert hasattr(lib, name), name
    for name in ("t5_decode_cross_attention_split", "t5_decode_cross_attention_split_plan",
                 "t5_decode_cross_attention_split_geometry"):
        assert name in P.__all__ and getattr(P, name) is getattr(P.t5_decode, name)
    assert list(inspect.signature(P.t5_decode_cross_attention_split).parameters) == [
        "q", "k_enc", "v_enc", "key_mask", "live", "n_heads", "groups", "splits", "workspace"]
    # the existing calls keep their signatures
    assert list(inspect.signature(P.t5_decode_cross_attention_grouped).parameters) == [
        "q", "k_enc", "v_enc", "key_mask", "live", "n_heads"]
    assert P.t5_decode.SPLIT_MAX == S.CAP


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("dtype,d", GEOMETRIES)
def test_geometry_ranges_are_whole_rounds_of_the_groups_and_cover_the_keys(dtype, d):
    want_ng = {(torch.bfloat16, 64): 32, (torch.bfloat16, 128): 16, (torch.float32, 64): 16, (torch.float32, 128): 8}[dtype, d]
    for Sn in sorted(set(S.SS) | set(range(1, 70)) | {127, 128, 129, 255, 256, 511, 512, 513, 2048, 4097}):
        for X in range(1, S.CAP + 1):
            g = P.t5_decode_cross_attention_split_geometry(dtype, d, Sn, X)
            assert g["NG"] == want_ng and g["max_splits"] == S.CAP and g["tile"] == 4
            assert g["C"] >= want_ng and g["C"] % g["NG"] == 0 and g["C"] * X >= Sn, (Sn, X, g)
            assert g["C"] - g["NG"] < -(-Sn // X), (Sn, X, g)                 # rounded up by less than one round
            assert 1 <= g["ranges"] <= X
            assert (g["ranges"] - 1) * g["C"] < Sn <= g["ranges"] * g["C"], (Sn, X, g)   # the non-empty ranges, no more
            assert {k: g[k] for k in ("NG", "C", "ranges")} == S.geometry(dtype, d, Sn, X)
    assert P.t5_decode_cross_attention_split_geometry(dtype, d, 1, 8)["ranges"] == 1


def test_geometry_reports_the_tile_cap_in_force():
    try:
        for tile in (1, 2, 8, 4):
            P.t5_decode.t5_decode_cross_attention_group_tile(tile)
            assert P.t5_decode_cross_attention_split_geometry(torch.bfloat16, 64, 200, 2)["tile"] == tile
    finally:
        P.t5_decode.t5_decode_cross_attention_group_tile(0)
    assert P.t5_decode_cross_attention_split_geometry(torch.bfloat16, 64, 200, 2)["tile"] == 4


def test_geometry_refusals():
    g = _lib.T5DecodeAttnSplitGeometry()
    for args in ((_lib.I64, 64, 9, 2), (77, 64, 9, 2), (_lib.BF16, 32, 9, 2), (_lib.BF16, 96, 9, 2), (_lib.BF16, 64, 0, 2),
                 (_lib.BF16, 64, -1, 2), (_lib.BF16, 64, 1 << 25, 2), (_lib.BF16, 64, 9, 0), (_lib.BF16, 64, 9, -1),
                 (_lib.BF16, 64, 9, S.CAP + 1)):
        g.NG = g.C = g.ranges = 7
        assert _lib.query("trlx_t5_decode_attn_split_geometry", *args, ctypes.byref(g)) == C.ERR_ARG, args
        assert "split decode attention geometry" in _lib.query("trlx_last_error").decode()
        assert (g.NG, g.C, g.ranges) == (0, 0, 0)
    assert _lib.query("trlx_t5_decode_attn_split_geometry", _lib.BF16, 64, 9, 2, None) == C.ERR_ARG
    with pytest.raises(ValueError):
        P.t5_decode_cross_attention_split_geometry(torch.float16, 64, 9, 2)


# ------------------------------------------------------------------ workspace
def test_workspace_bytes_grow_exactly_with_rows_heads_and_splits():
    f = P.t5_decode.t5_decode_cross_attention_split_workspace_bytes
    for d in (64, 128):
        unit = (d + 2) * 4                                           # M, L and d_kv floats
        assert f(1, 1, d, 1) == unit
        prev = 0
        for rows in (1, 2, 7, 256):
            for nH in (1, 5, 12, 32):
                for X in range(1, S.CAP + 1):
                    assert f(rows, nH, d, X) == rows * nH * X * unit
        for X in range(1, S.CAP + 1):                                # monotone in each argument
            assert f(8, 12, d, X) > prev
            prev = f(8, 12, d, X)
        assert f(9, 12, d, 4) > f(8, 12, d, 4) and f(8, 13, d, 4) > f(8, 12, d, 4)
    for bad in ((0, 1, 64, 1), (1, 0, 64, 1), (1, 1, 32, 1), (1, 1, 64, 0), (1, 1, 64, S.CAP + 1), (-1, 1, 64, 1),
                (1 << 33, 1, 64, 1), (1 << 20, 1 << 12, 64, 1)):
        assert f(*bad) == 0, bad


# ------------------------------------------------------------------ plan
def test_the_plan_is_a_deterministic_function_of_the_shape_inside_the_range():
    plan = P.t5_decode_cross_attention_split_plan
    shapes = [(dt, Pn, G, nH, d, Sn) for dt in (torch.bfloat16, torch.float32)
              for Pn, G in ((1, 1), (8, 1), (2, 4), (64, 4), (32, 8), (256, 1), (128, 1), (1024, 1))
              for nH, d in ((12, 64), (32, 128), (1, 64)) for Sn in (1, 9, 128, 512, 2048, 8192)]
    first = [plan(*s) for s in shapes]
    assert all(1 <= x <= S.CAP for x in first)
    assert [plan(*s) for s in reversed(shapes)] == first[::-1]        # no state between calls
    try:                                                              # the tile knob is not an argument of the plan
        P.t5_decode.t5_decode_cross_attention_group_tile(8)
        assert [plan(*s) for s in shapes] == first
    finally:
        P.t5_decode.t5_decode_cross_attention_group_tile(0)
    # arguments the entry would refuse: 1, never an error
    for bad in ((_lib.I64, 8, 1, 12, 64, 512), (_lib.BF16, 8, 1, 12, 96, 512), (_lib.BF16, 0, 1, 12, 64, 512),
                (_lib.BF16, 8, 0, 12, 64, 512), (_lib.BF16, 8, 1, 0, 64, 512), (_lib.BF16, 8, 1, 12, 64, 0)):
        assert _lib.query("trlx_t5_decode_attn_split_plan", *bad) == 1, bad
    assert plan(torch.float16, 8, 1, 12, 64, 512) == 1


# ------------------------------------------------------------------ refusals
def split_args(**over):
    """A legal call at P 3, G 4, nH 5, d 64, S 9, bf16, contiguous [P, nH, S, d], on dummy addresses."""
    nH, d, Sn = 5, 64, 9
    f = dict(q=BASE, ldq=nH * d, k=BASE + (1 << 24), k_stride_p=nH * Sn * d, k_stride_h=Sn * d, k_stride_s=d,
             v=BASE + (2 << 24), v_stride_p=nH * Sn * d, v_stride_h=Sn * d, v_stride_s=d, key_mask=BASE + (3 << 24),
             live=BASE + (4 << 24), out=BASE + (5 << 24), P=3, G=4, n_heads=nH, d_kv=d, S=Sn, dtype=_lib.BF16)
    f.update(over)
    return _lib.T5DecodeAttnGroupArgs(**f)


NEED = 12 * 5 * 2 * 66 * 4     # the legal call at two splits

# everything the grouped entry refuses (tests/test_t5_cross_group_cpu.py) and the merge's own grid limit (the last
# line), here with a legal workspace
REFUSED_AS_GROUPED = [
    ("NULL q", dict(q=None)), ("NULL k", dict(k=None)), ("NULL v", dict(v=None)), ("NULL out", dict(out=None)),
    ("an int64 dtype", dict(dtype=_lib.I64)), ("an unknown dtype", dict(dtype=77)),
    ("d_kv 32", dict(d_kv=32)), ("d_kv 96", dict(d_kv=96)), ("d_kv 256", dict(d_kv=256)),
    ("P 0", dict(P=0)), ("G 0", dict(G=0)), ("G -1", dict(G=-1)), ("n_heads 0", dict(n_heads=0)), ("S 0", dict(S=0)),
    ("ldq below nH * d", dict(ldq=5 * 64 - 8)), ("ldq not whole vectors", dict(ldq=5 * 64 + 4)),
    ("fp32 ldq not whole vectors", dict(dtype=_lib.F32, ldq=5 * 64 + 2)),
    ("a negative prompt stride", dict(k_stride_p=-5 * 9 * 64)), ("a negative key stride", dict(v_stride_s=-64)),
    ("a prompt stride not whole vectors", dict(k_stride_p=5 * 9 * 64 + 4)),
    ("a head stride not whole vectors", dict(v_stride_h=9 * 64 + 2)),
    ("a key stride not whole vectors", dict(k_stride_s=64 + 12)),
    ("an fp32 stride not whole vectors", dict(dtype=_lib.F32, v_stride_p=5 * 9 * 64 + 2)),
    ("a head stride below d_kv", dict(k_stride_h=32)), ("a value head stride below d_kv", dict(v_stride_h=56)),
    ("a key stride below d_kv", dict(k_stride_s=56)), ("a value key stride below d_kv", dict(v_stride_s=0)),
    ("q off 16 bytes", dict(q=BASE + 8)), ("k off 16 bytes", dict(k=BASE + (1 << 24) + 2)),
    ("v off 16 bytes", dict(v=BASE + (2 << 24) + 4)), ("out off 16 bytes", dict(out=BASE + (5 << 24) + 8)),
    ("the mask off 8 bytes", dict(key_mask=BASE + (3 << 24) + 4)), ("live off 8 bytes", dict(live=BASE + (4 << 24) + 4)),
    ("P * n_heads past the grid", dict(P=1 << 30, n_heads=4)), ("P past 32 bits", dict(P=1 << 33)),
    ("rows past 32 bits", dict(P=1 << 20, G=1 << 12)), ("too many query tiles", dict(P=1, G=1 << 20)),
    ("S past 2^31 / 128", dict(S=1 << 25)), ("n_heads past 2^31 / 128", dict(P=1, n_heads=1 << 25)),
    ("rows * n_heads past 32 bits", dict(P=1 << 16, G=1 << 8, n_heads=1 << 8)),
]


@pytest.mark.parametrize("name,over", REFUSED_AS_GROUPED, ids=[n for n, _ in REFUSED_AS_GROUPED])
@pytest.mark.parametrize("splits", (0, 1, 2, 8))
def test_everything_the_grouped_entry_refuses_is_refused_before_any_launch(name, over, splits):
    a = split_args(**over)
    assert _lib.query("trlx_t5_decode_attn_split", ctypes.byref(a), splits, WS, 1 << 40, None) == C.ERR_ARG, name
    assert "split decode attention" in _lib.query("trlx_last_error").decode()


REFUSED_OWN = [
    ("splits -1", dict(splits=-1)), ("splits past the cap", dict(splits=S.CAP + 1)), ("splits 64", dict(splits=64)),
    ("a NULL workspace", dict(ws=None)), ("a NULL workspace at one split", dict(ws=None, splits=1)),
    ("a NULL workspace under the plan", dict(ws=None, splits=0)),
    ("a workspace off 16 bytes", dict(ws=WS + 8)), ("a workspace off 4 bytes", dict(ws=WS + 4)),
    ("a workspace one byte short", dict(nbytes=NEED - 1)), ("an empty workspace", dict(nbytes=0)),
    ("a negative workspace size", dict(nbytes=-1)),
    ("a workspace sized for fewer splits", dict(splits=4, nbytes=NEED)),
    ("a workspace one byte short at one split", dict(splits=1, nbytes=NEED // 2 - 1)),
]


@pytest.mark.parametrize("name,over", REFUSED_OWN, ids=[n for n, _ in REFUSED_OWN])
def test_splits_outside_the_range_and_bad_workspaces_are_refused_before_any_launch(name, over):
    f = dict(splits=2, ws=WS, nbytes=NEED)
    f.update(over)
    a = split_args()
    assert _lib.query("trlx_t5_decode_attn_split", ctypes.byref(a), f["splits"], f["ws"], f["nbytes"], None) == C.ERR_ARG, name
    msg = _lib.query("trlx_last_error").decode()
    assert "split decode attention" in msg and ("splits" in msg or "workspace" in msg), msg


def test_null_arguments_are_refused():
    assert _lib.query("trlx_t5_decode_attn_split", None, 2, WS, 1 << 40, None) == C.ERR_ARG
    assert "NULL arguments" in _lib.query("trlx_last_error").decode()


# ------------------------------------------------------------------ the wrapper
def test_the_wrappers_shape_errors_and_its_fall_back_off_the_device():
    d, Sn, Gn = 64, 9, 4
    c = S.group_case(torch.bfloat16, d, Sn, "right", Gn)
    q, K, V, mask = c["q"], c["K"], c["V"], c["mask"]
    f = P.t5_decode_cross_attention_split
    with pytest.raises(ValueError, match="prompts \\* groups"):
        f(q, K, V, groups=3)
    with pytest.raises(ValueError, match="prompts \\* groups"):
        f(q, K, V)                                                   # groups defaults to 1: 12 rows over 3 prompts
    with pytest.raises(ValueError, match="prompts \\* groups"):
        f(q, K, V, groups=0)
    for bad in (0, -1, S.CAP + 1):
        with pytest.raises(ValueError, match="splits"):
            f(q, K, V, groups=Gn, splits=bad)
    with pytest.raises(ValueError, match="n_heads"):
        f(q, K.permute(0, 2, 1, 3).reshape(S.P, Sn, S.NH * d), V.permute(0, 2, 1, 3).reshape(S.P, Sn, S.NH * d), groups=Gn)
    with pytest.raises(ValueError):
        f(q, K, V.float(), groups=Gn)
    with pytest.raises(ValueError):
        f(q.float(), K, V, groups=Gn)
    with pytest.raises(ValueError, match="key_mask"):
        f(q, K, V, mask.repeat_interleave(Gn, 0), groups=Gn)         # the mask is per prompt
    with pytest.raises(ValueError, match="live"):
        f(q, K, V, mask, live=torch.ones(S.P, dtype=torch.int64), groups=Gn)
    with pytest.raises(TypeError):
        f(q, [K], [V], groups=Gn)
    # off the device the call does what the grouped one does
    with pytest.raises(ValueError) as mine:
        f(q, K, V, mask, groups=Gn, splits=2)
    with pytest.raises(ValueError) as theirs:
        P.t5_decode_cross_attention_grouped(q, K, V, mask)
    assert str(mine.value) == str(theirs.value)
    h = dict(q=q.to(torch.float16), K=K.to(torch.float16), V=V.to(torch.float16))   # a dtype the kernels do not take
    want = P.t5_decode_cross_attention_grouped(h["q"], h["K"], h["V"], mask)
    for X in (None, 1, 4):
        assert C.same(f(h["q"], h["K"], h["V"], mask, groups=Gn, splits=X), want)
