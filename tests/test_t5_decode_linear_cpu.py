"""t5_decode_linear without a GPU: the torch route against the float64 oracle, the argument checks,
T5DecodeBlockWeights.from_state_dict, and the binding against the header."""
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


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_the_torch_route_on_a_cpu_matches_the_float64_oracle(combo, dtype):
    norm, (_, with_res, act, gated) = combo
    for M, N, K in ((1, 16, 32), (3, 48, 96), (17, 24, 40)):      # the last is off the kernel's grid
        x, w, nw, res = (t.to(dtype) for t in L.inputs(M, N, K, gated, seed=K + M))
        x[:2] = torch.randn(min(M, 2), K, generator=torch.Generator().manual_seed(M)).to(dtype)   # rows of one scale
        got = P.t5_decode_linear(x, w, norm_weight=nw if norm else None, residual=res if with_res else None, act=act,
                                 gated=gated)
        ref = L.oracle(x, w, nw if norm else None, 1e-6, res if with_res else None, act, gated)
        assert got.shape == (M, N) and got.dtype == dtype
        # every op of the route rounds once to `dtype`: a few ulps of the largest value it forms
        eps = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22
        scale = float(ref.abs().max()) + float(L.oracle(x, w, nw if norm else None).abs().max())
        assert L.max_err(got, ref) <= 8 * eps * scale, (M, N, K)


def test_out_and_3d_rows_on_a_cpu():
    x, w, _, res = L.inputs(3, 16, 32, False, seed=1)
    want = P.t5_decode_linear(x, w, residual=res)
    out = torch.empty(3, 16, dtype=x.dtype)
    assert P.t5_decode_linear(x, w, residual=res, out=out) is out and torch.equal(out, want)
    got3 = P.t5_decode_linear(x[:, None, :], w)
    assert got3.shape == (3, 1, 16) and torch.equal(got3[:, 0], P.t5_decode_linear(x, w))
    r = res.clone()
    P.t5_decode_linear(x, w, residual=r, out=r)                   # in place
    assert torch.equal(r, want)


def test_argument_checks():
    x, w, nw, res = L.inputs(3, 16, 32, True, seed=2)
    with pytest.raises(ValueError, match="forward only"):
        P.t5_decode_linear(x.clone().requires_grad_(True), w[:16])
    with torch.no_grad():                                         # under no_grad a parameter is fine
        P.t5_decode_linear(x, torch.nn.Parameter(w[:16]))
    for bad in (dict(residual=res, act="silu"), dict(gated=True), dict(act="gelu"), dict(norm_weight=nw[:16]),
                dict(residual=res[:, :8]), dict(out=torch.empty(3, 8, dtype=x.dtype)), dict(norm_weight=nw.float())):
        with pytest.raises(ValueError):
            P.t5_decode_linear(x, w[:16], **bad)
    with pytest.raises(ValueError):
        P.t5_decode_linear(x, w[:17], act="silu", gated=True)     # an odd number of rows cannot be [2F, K]
    with pytest.raises(ValueError):
        P.t5_decode_linear(x[None, None], w[:16])
    with pytest.raises(TypeError):
        P.t5_decode_linear(x, [1, 2])


@pytest.mark.parametrize("gated", (True, False), ids=("gated", "plain"))
def test_from_state_dict_packs_in_order_round_trips_and_refuses_a_missing_key(gated):
    D, inner, F = 32, 48, 80
    prefix = "decoder.block.3."
    sd = L.hf_block_state_dict(D, inner, F, gated, seed=4, prefix=prefix)
    w = P.T5DecodeBlockWeights.from_state_dict(sd, prefix, gated=gated)
    assert (w.inner, w.d_model, w.d_ff, w.gated) == (inner, D, F, gated)
    assert w.qkv.shape == (3 * inner, D) and w.qkv.is_contiguous()
    for j, n in enumerate("qkv"):
        assert torch.equal(w.qkv[j * inner:(j + 1) * inner], sd[prefix + f"layer.0.SelfAttention.{n}.weight"])
    assert w.o.shape == (D, inner) and w.cq.shape == (inner, D) and w.co.shape == (D, inner) and w.wo.shape == (D, F)
    if gated:
        assert w.wi.shape == (2 * F, D)
        assert torch.equal(w.wi[:F], sd[prefix + "layer.2.DenseReluDense.wi_0.weight"])
        assert torch.equal(w.wi[F:], sd[prefix + "layer.2.DenseReluDense.wi_1.weight"])
    else:
        assert w.wi.shape == (F, D)
    assert len(w.ln) == 3 and all(g.shape == (D,) for g in w.ln)
    # back to HF's names: every key a decode step uses, bit for bit
    back = w.state_dict(prefix)
    unused = {prefix + f"layer.1.EncDecAttention.{n}.weight" for n in "kv"} | \
             {prefix + "layer.0.SelfAttention.relative_attention_bias.weight"}
    assert set(back) == set(sd) - unused
    for k, v in back.items():
        assert torch.equal(v, sd[k]), k
    # the packed output slices are what the attention reads: x @ qkv.T = [x @ q.T | x @ k.T | x @ v.T]
    x = torch.randn(2, D).to(torch.bfloat16)
    z = P.t5_decode_linear(x, w.qkv)
    for j, n in enumerate("qkv"):
        assert torch.equal(z[:, j * inner:(j + 1) * inner], torch.nn.functional.linear(x, sd[prefix + f"layer.0.SelfAttention.{n}.weight"]))
    for k in back:
        broken = dict(sd)
        del broken[k]
        with pytest.raises(KeyError, match=re.escape(k)):
            P.T5DecodeBlockWeights.from_state_dict(broken, prefix, gated=gated)
    with pytest.raises(KeyError):                                 # the other feed-forward form's names
        P.T5DecodeBlockWeights.from_state_dict(sd, prefix, gated=not gated)


def test_the_fused_layer_on_a_cpu_is_the_sequence_of_its_parts():
    D, inner, F = 32, 64, 48
    w = P.T5DecodeBlockWeights.from_state_dict(L.hf_block_state_dict(D, inner, F, True, seed=5), "decoder.block.0.")
    h0 = torch.randn(3, D, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    sa = lambda q, k, v: (q.float() + k.float() - v.float()).to(q.dtype)
    ca = lambda q: (q.float() * 0.5).to(q.dtype)
    h = h0.clone()
    assert P.t5_decode_layer_fused(h, w, sa, ca) is h
    want = h0.clone()
    qkv = P.t5_decode_linear(want, w.qkv, norm_weight=w.ln[0])
    want = P.t5_decode_linear(sa(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:]), w.o, residual=want)
    want = P.t5_decode_linear(ca(P.t5_decode_linear(want, w.cq, norm_weight=w.ln[1])), w.co, residual=want)
    f = P.t5_decode_linear(want, w.wi, norm_weight=w.ln[2], act="gelu_new", gated=True)
    want = P.t5_decode_linear(f, w.wo, residual=want)
    assert torch.equal(h, want)


def test_the_binding_mirrors_the_header():
    header = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    body = re.search(r"typedef struct trlx_t5_decode_linear_args \{(.*?)\} trlx_t5_decode_linear_args;", header, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in _lib.T5DecodeLinearArgs._fields_]
    gbody = re.search(r"typedef struct TrlxT5DecodeLinearGeometry \{(.*?)\} TrlxT5DecodeLinearGeometry;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", gbody, flags=re.S)) == [n for n, _ in _lib.T5DecodeLinearGeometry._fields_]
    assert _lib.SIGNATURES["trlx_t5_decode_linear"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeLinearArgs), ctypes.c_void_p])
    assert re.search(r"#define TRLX_T5_ACT_NONE \((-?\d+)\)", header).group(1) == str(_lib.T5_ACT_NONE)
    assert "t5_decode_linear.hip" in open(os.path.join(ROOT, "trlx-t5_amd", "csrc", "Makefile")).read()
    for name in ("t5_decode_linear", "T5DecodeBlockWeights", "t5_decode_layer_fused"):
        assert name in P.__all__ and hasattr(P, name)


def test_geometry_matches_the_constants_the_python_entry_dispatches_on():
    g = TDL.geometry()                                            # a host call: needs the library, no device
    assert g["cols_per_block"] == TDL.COLS_PER_BLOCK and g["k_per_chunk"] == TDL.K_PER_CHUNK
    assert g["max_k"] == TDL.MAX_K and g["norm_max_k"] == TDL.NORM_MAX_K == L.NORM_MAX_K
    # the breaks the tests straddle are the kernel's: the waves' K split and the norm's forms
    turn = g["k_per_chunk"] * g["chunks_per_wave_turn"]
    waves = g["threads"] // 64
    assert [turn * (i + 1) for i in range(waves)] == sorted(L.K_BREAKS)[:waves]
    assert g["norm_wave_row_max_k"] in L.K_BREAKS and g["norm_max_k"] in L.K_BREAKS
    tiles = g["max_row_tiles"] * g["rows_per_tile"]
    assert L.M_BREAKS == (tiles // 4 + 1, tiles // 2 + 1, tiles + 1)
    assert L.K_LARGEST[2] == g["max_k"]
