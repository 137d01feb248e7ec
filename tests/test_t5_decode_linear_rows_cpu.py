"""t5_decode_linear(live=, split_rows=) without a GPU: the binding against the header, the geometry,
the torch route's dead-row rule for every combination, the fused layer with `live`, and the argument
checks."""
import ctypes
import os
import re
import sys

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_decode_linear_checks as L

TDL = sys.modules["trlx_t5_amd.t5_decode_linear"]   # the module: the package attribute of that name is the function
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    return re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_the_binding_mirrors_the_header():
    header = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    fields = struct_fields(header, "trlx_t5_decode_linear_rows_args")
    assert fields == [n for n, _ in _lib.T5DecodeLinearRowsArgs._fields_]
    # the existing fields in the existing order, then live and a reserved word
    old = struct_fields(header, "trlx_t5_decode_linear_args")
    assert fields == old + ["live", "reserved"]
    assert _lib.T5DecodeLinearRowsArgs._fields_[:len(old)] == _lib.T5DecodeLinearArgs._fields_
    assert dict(_lib.T5DecodeLinearRowsArgs._fields_)["live"] is ctypes.c_void_p
    assert dict(_lib.T5DecodeLinearRowsArgs._fields_)["reserved"] is ctypes.c_int64
    assert struct_fields(header, "TrlxT5DecodeLinearRowsGeometry") == [n for n, _ in _lib.T5DecodeLinearRowsGeometry._fields_]
    assert struct_fields(header, "TrlxT5DecodeLinearRowsGeometry") == ["threads", "cols_per_block", "rows_per_tile",
                                                                       "rows_per_block", "max_m_live", "reserved"]
    assert re.search(r"int trlx_t5_decode_linear_rows\(const trlx_t5_decode_linear_rows_args\* a, void\* stream\);", header)
    assert re.search(r"int trlx_t5_decode_linear_rows_geometry\(TrlxT5DecodeLinearRowsGeometry\* g\);", header)
    assert _lib.SIGNATURES["trlx_t5_decode_linear_rows"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeLinearRowsArgs),
                                                                            ctypes.c_void_p])
    assert _lib.SIGNATURES["trlx_t5_decode_linear_rows_geometry"] == (ctypes.c_int,
                                                                     [ctypes.POINTER(_lib.T5DecodeLinearRowsGeometry)])
    makefile = open(os.path.join(ROOT, "trlx-t5_amd", "csrc", "Makefile")).read()
    assert "t5_decode_linear_rows.hip" in makefile.split("SRCS")[1].splitlines()[0]


def test_rows_geometry_agrees_with_the_constants_the_tests_straddle():
    g = TDL.rows_geometry()                                       # a host call: needs the library, no device
    old = TDL.geometry()
    assert g["threads"] == old["threads"] and g["cols_per_block"] == old["cols_per_block"] == TDL.COLS_PER_BLOCK
    assert g["rows_per_tile"] == old["rows_per_tile"]
    assert g["rows_per_block"] == TDL.ROWS_PER_BLOCK and g["max_m_live"] == TDL.MAX_M_LIVE
    # the gated form's two slabs of rows_per_block / rows_per_tile tiles fit a wave's accumulator tiles
    assert g["rows_per_block"] % g["rows_per_tile"] == 0
    assert 2 * g["rows_per_block"] // g["rows_per_tile"] <= old["max_row_tiles"]
    assert g["max_m_live"] >= 256 and g["max_m_live"] % g["rows_per_block"] == 0
    assert "reserved" not in g


def mixed_live(M, seed):
    """Some rows live and some dead, whatever M >= 2 (M 1: the one row dead)."""
    live = (torch.rand(M, generator=torch.Generator().manual_seed(seed)) < 0.5).to(torch.int64) * 3   # nonzero = live
    if M >= 2:
        live[0], live[-1] = 0, 7
    else:
        live[0] = 0
    return live


@pytest.mark.parametrize("dtype", (torch.float32, BF), ids=("fp32", "bf16"))
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_the_torch_route_on_a_cpu_follows_the_dead_row_rule(combo, dtype):
    norm, (_, with_res, act, gated) = combo
    for M, N, K in ((1, 16, 32), (5, 48, 96), (17, 24, 40)):      # the last is off the kernel's grid
        x, w, nw, res = (t.to(dtype) for t in L.inputs(M, N, K, gated, seed=K + M))
        kw = dict(norm_weight=nw if norm else None, residual=res if with_res else None, act=act, gated=gated)
        want = P.t5_decode_linear(x, w, **kw)
        live = mixed_live(M, seed=M)
        on = live != 0
        got = P.t5_decode_linear(x, w, live=live, **kw)
        assert got.shape == (M, N) and got.dtype == dtype
        assert torch.equal(got[on], want[on]), (M, N, K, "live rows")
        dead = res[~on] if with_res else torch.zeros_like(got[~on])
        assert torch.equal(got[~on], dead), (M, N, K, "dead rows")
        # all live and split_rows alone: the call without either
        assert torch.equal(P.t5_decode_linear(x, w, live=torch.ones(M, dtype=torch.int64), **kw), want)
        assert torch.equal(P.t5_decode_linear(x, w, split_rows=True, **kw), want)
        # a preallocated out
        out = torch.full((M, N), 5.0, dtype=dtype)
        assert P.t5_decode_linear(x, w, live=live, out=out, **kw) is out and torch.equal(out, got)
        if with_res:                                              # in place: a dead row is left untouched
            r = res.clone()
            assert P.t5_decode_linear(x, w, live=live, **dict(kw, residual=r), out=r) is r
            assert torch.equal(r[on], want[on]) and torch.equal(r[~on], res[~on])
        assert live.tolist() == mixed_live(M, seed=M).tolist()    # live is read only


def test_the_fused_layer_with_live_on_a_cpu_is_the_sequence_of_its_parts():
    D, inner, F = 32, 64, 48
    w = P.T5DecodeBlockWeights.from_state_dict(L.hf_block_state_dict(D, inner, F, True, seed=5), "decoder.block.0.")
    h0 = torch.randn(5, D, generator=torch.Generator().manual_seed(1)).to(BF)
    live = torch.tensor([1, 0, 2, 0, 1])
    on = live != 0
    sa = lambda q, k, v: (q.float() + k.float() - v.float()).to(q.dtype)
    ca = lambda q: (q.float() * 0.5).to(q.dtype)
    h = h0.clone()
    bufs = dict(qkv=torch.empty(5, 3 * inner, dtype=BF), cq=torch.empty(5, inner, dtype=BF), ff=torch.empty(5, F, dtype=BF))
    assert P.t5_decode_layer_fused(h, w, sa, ca, bufs=bufs, live=live, split_rows=True) is h
    kw = dict(live=live, split_rows=True)
    want = h0.clone()
    qkv = P.t5_decode_linear(want, w.qkv, norm_weight=w.ln[0], **kw)
    want = P.t5_decode_linear(sa(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:]), w.o, residual=want, **kw)
    cq = P.t5_decode_linear(want, w.cq, norm_weight=w.ln[1], **kw)
    want = P.t5_decode_linear(ca(cq), w.co, residual=want, **kw)
    f = P.t5_decode_linear(want, w.wi, norm_weight=w.ln[2], act="gelu_new", gated=True, **kw)
    want = P.t5_decode_linear(f, w.wo, residual=want, **kw)
    assert torch.equal(h, want)
    assert torch.equal(bufs["qkv"], qkv) and torch.equal(bufs["cq"], cq) and torch.equal(bufs["ff"], f)
    # a live row is the layer without live; a dead row of the stream is left as it was, its buffers are zeros
    plain = h0.clone()
    P.t5_decode_layer_fused(plain, w, sa, ca)
    assert torch.equal(h[on], plain[on]) and torch.equal(h[~on], h0[~on])
    for b in bufs.values():
        assert not b[~on].any()
    # the defaults are the call as it was
    again = h0.clone()
    P.t5_decode_layer_fused(again, w, sa, ca, live=None, split_rows=False)
    assert torch.equal(again, plain)


def test_argument_checks_of_live():
    x, w, _, res = L.inputs(4, 16, 32, False, seed=2)
    good = torch.ones(4, dtype=torch.int64)
    P.t5_decode_linear(x, w, live=good)
    bad = (torch.ones(4, dtype=torch.int32), torch.ones(4, dtype=torch.bool), torch.ones(4), torch.ones(5, dtype=torch.int64),
           torch.ones(3, dtype=torch.int64), torch.ones(4, 1, dtype=torch.int64), torch.ones(8, dtype=torch.int64)[::2],
           torch.ones(4, dtype=torch.int64, device="meta"), [1, 1, 1, 1])
    for live in bad:
        with pytest.raises(ValueError, match="live"):
            P.t5_decode_linear(x, w, live=live)
        with pytest.raises(ValueError, match="live"):
            P.t5_decode_linear(x, w, residual=res, live=live, split_rows=True)
    for name in ("rows_geometry", "ROWS_PER_BLOCK", "MAX_M_LIVE"):
        assert name in TDL.__all__ and hasattr(TDL, name)
