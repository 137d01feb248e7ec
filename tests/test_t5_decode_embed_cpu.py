"""t5_decode_embed and the live-row entry without a GPU: the header's declarations, the ctypes mirror,
the binding's symbol list, the package export and the torch fallback on a CPU device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_rollout_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()


def test_the_header_declares_the_two_entries_and_the_struct():
    flat = re.sub(r"\s+", " ", HEADER)
    for decl in ("int trlx_t5_decode_embed(const TrlxT5DecodeEmbedArgs* a, const int64_t* clock, void* stream);",
                 "int trlx_t5_decode_attn_live(const TrlxT5DecodeAttnArgs* a, const int64_t* live, const int64_t* clock, "
                 "void* stream);",
                 "typedef struct TrlxT5DecodeEmbedArgs {", "} TrlxT5DecodeEmbedArgs;"):
        assert decl in flat, decl
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", HEADER) and _lib.ABI_VERSION == 2


def test_the_ctypes_mirror_has_the_headers_field_order_and_types():
    body = re.search(r"typedef struct TrlxT5DecodeEmbedArgs \{(.*?)\} TrlxT5DecodeEmbedArgs;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.match(r"(.*?)(\w+)$", f.strip()).groups() for f in body.split(";") if f.strip()]
    assert [n for _, n in fields] == [n for n, _ in _lib.T5DecodeEmbedArgs._fields_]
    for (ctype, fname), (_, py) in zip(fields, _lib.T5DecodeEmbedArgs._fields_):
        want = ctypes.c_void_p if "*" in ctype else {"int64_t": ctypes.c_int64, "float": ctypes.c_float,
                                                     "int": ctypes.c_int}[ctype.strip()]
        assert py is want, (ctype, fname)
    assert ctypes.sizeof(_lib.T5DecodeEmbedArgs) == 15 * 8 + 4 + 4


def test_the_binding_lists_the_new_symbols_and_the_package_exports_the_wrapper():
    sig = _lib.SIGNATURES
    vp = ctypes.c_void_p
    assert sig["trlx_t5_decode_embed"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeEmbedArgs), vp, vp])
    assert sig["trlx_t5_decode_attn_live"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeAttnArgs), vp, vp, vp])
    assert "t5_decode_embed" in P.__all__ and P.t5_decode_embed is P.t5_decode.t5_decode_embed
    assert list(inspect.signature(P.t5_decode_embed).parameters) == ["weight", "tokens", "t", "start_token_id",
                                                                     "norm_weight", "eps", "out"]
    for fn in (P.t5_decode_self_attention, P.t5_decode_cross_attention):
        assert inspect.signature(fn).parameters["live"].default is None


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=C.name)
def test_the_cpu_fallback_is_the_embedding_and_the_layer_norm(dtype):
    g = torch.Generator().manual_seed(11)
    B, T, V, D, start = 5, 6, 37, 96, 3
    weight = torch.randn(V, D, generator=g).to(dtype)
    norm_w = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dtype)
    tokens = torch.randint(0, V, (B, T), generator=g)
    tokens[0, 0], tokens[1, 0], tokens[2, 0], tokens[3, 0] = 0, V - 1, -1, V     # the edges and two ids out of range
    for t in (0, 1, T):
        h, y = P.t5_decode_embed(weight, tokens, t, start, norm_w)
        want = C.embed_reference(weight, tokens, t, start)
        assert C.same(h, want) and C.same(y, C.hf_layer_norm(want, norm_w)), t
        h2, y2 = P.t5_decode_embed(weight, tokens, t, start)
        assert y2 is None and C.same(h2, want)
    h0, _ = P.t5_decode_embed(weight, tokens, 0, start, norm_w)
    assert C.same(h0, weight[start].expand(B, D))                                 # t == 0: the start token in every row
    h1, y1 = P.t5_decode_embed(weight, tokens, 1, start, norm_w)
    assert not h1[2].any() and not h1[3].any() and not y1[2].any()               # ids -1 and V: zero rows
    assert C.same(h1[0], weight[0]) and C.same(h1[1], weight[V - 1])
    # out= is written in place; a recorder stands for its tokens
    out = (torch.full((B, D), C.GUARD, dtype=dtype), torch.full((B, D), C.GUARD, dtype=dtype))
    got = P.t5_decode_embed(weight, tokens, 1, start, norm_w, out=out)
    assert got[0] is out[0] and got[1] is out[1] and C.same(out[0], h1) and C.same(out[1], y1)
    rec = P.PPORolloutRecorder(B, T, "cpu", pad_token_id=0, eos_token_id=1)
    rec.tokens.copy_(tokens)
    assert C.same(P.t5_decode_embed(weight, rec, 1, start)[0], h1)


def test_refusals_that_need_no_device():
    weight, tokens = torch.zeros(7, 8), torch.zeros(2, 3, dtype=torch.int64)
    for bad_t in (-1, 4):
        with pytest.raises(ValueError, match="outside"):
            P.t5_decode_embed(weight, tokens, bad_t, 0)
    with pytest.raises(ValueError, match="tokens"):
        P.t5_decode_embed(weight, tokens.int(), 0, 0)
    with pytest.raises(ValueError, match="norm_weight"):
        P.t5_decode_embed(weight, tokens, 0, 0, torch.zeros(9))
    with pytest.raises(ValueError, match="out"):
        P.t5_decode_embed(weight, tokens, 0, 0, out=(torch.zeros(2, 8), torch.zeros(2, 8)))
    with pytest.raises(ValueError, match="captured"):
        P.t5_decode_embed(weight, tokens, P.T5DecodeClock(3, "cpu"), 0)
    # live= is checked before anything else is done with it
    cache = P.T5DecodeKVCache(2, 1, 64, 4, torch.float32, "cpu")
    q = torch.zeros(2, 64)
    for live in (torch.ones(2, dtype=torch.int32), torch.ones(3, dtype=torch.int64), torch.ones(4, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match="live"):
            P.t5_decode_self_attention(q, q, q, cache, 0, live=live)
        with pytest.raises(ValueError, match="live"):
            P.t5_decode_cross_attention(q, cache.k, cache.v, live=live)
