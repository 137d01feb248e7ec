"""The grouped decode cross-attention without a GPU: the header's declarations, the ctypes mirror, the
binding's symbol list, the package export, every refusal of trlx_t5_decode_attn_group (each returns
before any launch, so aligned dummy addresses stand for device memory) and the wrapper's shape errors."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_cross_group_checks as G
import t5_rollout_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
BASE = 0x7f0000000000          # never dereferenced: every call below is refused before a launch


def test_the_header_declares_the_entry_and_the_struct_and_keeps_the_abi_version():
    flat = re.sub(r"\s+", " ", HEADER)
    for decl in ("int trlx_t5_decode_attn_group(const TrlxT5DecodeAttnGroupArgs* a, void* stream);",
                 "int trlx_t5_decode_attn_group_tile(int64_t tile);",
                 "typedef struct TrlxT5DecodeAttnGroupArgs {", "} TrlxT5DecodeAttnGroupArgs;"):
        assert decl in flat, decl
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", HEADER) and _lib.ABI_VERSION == 2
    assert _lib.query("trlx_abi_version") == 2


def test_the_ctypes_mirror_has_the_headers_field_order_types_and_size():
    body = re.search(r"typedef struct TrlxT5DecodeAttnGroupArgs \{(.*?)\} TrlxT5DecodeAttnGroupArgs;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (x.strip() for x in body.split(";") if x.strip()):      # `type a, b, c` declares three fields
        first, *more = decl.split(",")
        ctype, name = re.match(r"(.*?)(\w+)$", first.strip()).groups()
        fields += [(ctype.strip(), name)] + [(ctype.strip(), m.strip()) for m in more]
    assert [n for _, n in fields] == [n for n, _ in _lib.T5DecodeAttnGroupArgs._fields_]
    assert [n for _, n in fields] == ["q", "ldq", "k", "k_stride_p", "k_stride_h", "k_stride_s", "v", "v_stride_p",
                                      "v_stride_h", "v_stride_s", "key_mask", "live", "out", "P", "G", "n_heads",
                                      "d_kv", "S", "dtype"]
    for (ctype, name), (_, py) in zip(fields, _lib.T5DecodeAttnGroupArgs._fields_):
        want = ctypes.c_void_p if "*" in ctype else {"int64_t": ctypes.c_int64, "int": ctypes.c_int}[ctype]
        assert py is want, (ctype, name)
    assert ctypes.sizeof(_lib.T5DecodeAttnGroupArgs) == 18 * 8 + 4 + 4


def test_the_binding_lists_the_symbols_and_the_package_exports_the_wrapper():
    sig = _lib.SIGNATURES
    assert sig["trlx_t5_decode_attn_group"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeAttnGroupArgs), ctypes.c_void_p])
    assert sig["trlx_t5_decode_attn_group_tile"] == (ctypes.c_int, [ctypes.c_int64])
    lib = _lib.load()
    assert hasattr(lib, "trlx_t5_decode_attn_group") and hasattr(lib, "trlx_t5_decode_attn_group_tile")
    assert "t5_decode_cross_attention_grouped" in P.__all__
    assert P.t5_decode_cross_attention_grouped is P.t5_decode.t5_decode_cross_attention_grouped
    assert list(inspect.signature(P.t5_decode_cross_attention_grouped).parameters) == [
        "q", "k_enc", "v_enc", "key_mask", "live", "n_heads"]
    # the existing call keeps its signature
    assert list(inspect.signature(P.t5_decode_cross_attention).parameters) == ["q", "k_enc", "v_enc", "key_mask", "live"]


def group_args(**over):
    """A legal call at P 3, G 4, nH 5, d 64, S 9, bf16, contiguous [P, nH, S, d], on dummy addresses."""
    nH, d, S = 5, 64, 9
    f = dict(q=BASE, ldq=nH * d, k=BASE + (1 << 24), k_stride_p=nH * S * d, k_stride_h=S * d, k_stride_s=d,
             v=BASE + (2 << 24), v_stride_p=nH * S * d, v_stride_h=S * d, v_stride_s=d, key_mask=BASE + (3 << 24),
             live=BASE + (4 << 24), out=BASE + (5 << 24), P=3, G=4, n_heads=nH, d_kv=d, S=S, dtype=_lib.BF16)
    f.update(over)
    return _lib.T5DecodeAttnGroupArgs(**f)


REFUSED = [
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
]


@pytest.mark.parametrize("name,over", REFUSED, ids=[n for n, _ in REFUSED])
def test_every_refusal_comes_before_any_launch(name, over):
    a = group_args(**over)
    assert _lib.query("trlx_t5_decode_attn_group", ctypes.byref(a), None) == C.ERR_ARG, name
    assert "grouped decode attention" in _lib.query("trlx_last_error").decode()


def test_null_arguments_and_the_tile_knob_are_refused():
    assert _lib.query("trlx_t5_decode_attn_group", None, None) == C.ERR_ARG
    for tile in (-1, 3, 5, 16):
        assert _lib.query("trlx_t5_decode_attn_group_tile", tile) == C.ERR_ARG
    for tile in G.TILES + (0,):
        assert _lib.query("trlx_t5_decode_attn_group_tile", tile) == 0


def test_the_stride_of_a_dimension_of_size_one_is_not_read():
    """With P, n_heads or S = 1 (P * G = 1 for ldq) a wild stride there does not refuse the call: what
    does is the check that comes after the strides', the alignment of live, and its message is the
    one reported.  The same stride with that dimension above 1 is the strides' refusal."""
    bad_live = BASE + (4 << 24) + 4
    for over in (dict(P=1, G=12, k_stride_p=-3, v_stride_p=5), dict(n_heads=1, ldq=64, k_stride_h=7, v_stride_h=-1),
                 dict(S=1, k_stride_s=3, v_stride_s=-9), dict(P=1, G=1, ldq=-1)):
        a = group_args(live=bad_live, **over)
        assert _lib.query("trlx_t5_decode_attn_group", ctypes.byref(a), None) == C.ERR_ARG
        assert "8-byte aligned" in _lib.query("trlx_last_error").decode(), over
    for over in (dict(G=12, k_stride_p=-3), dict(ldq=5 * 64, k_stride_h=7), dict(k_stride_s=3), dict(ldq=-1)):
        a = group_args(live=bad_live, **over)
        assert _lib.query("trlx_t5_decode_attn_group", ctypes.byref(a), None) == C.ERR_ARG
        assert "stride" in _lib.query("trlx_last_error").decode(), over


def test_the_wrappers_shape_errors():
    d, S, Gn = 64, 9, 4
    c = G.group_case(torch.bfloat16, d, S, "right", Gn)
    q, K, V, mask = c["q"], c["K"], c["V"], c["mask"]
    f = P.t5_decode_cross_attention_grouped
    with pytest.raises(ValueError, match="whole multiple"):
        f(q[:-1], K, V)                                              # 11 rows over 3 prompts
    with pytest.raises(ValueError, match="whole multiple"):
        f(q[:2], K, V)                                               # fewer rows than prompts
    with pytest.raises(ValueError, match="n_heads"):
        f(q, K.permute(0, 2, 1, 3).reshape(G.P, S, G.NH * d), V.permute(0, 2, 1, 3).reshape(G.P, S, G.NH * d))
    with pytest.raises(ValueError, match="n_heads"):
        f(q, K.permute(0, 2, 1, 3).reshape(G.P, S, G.NH * d), V.permute(0, 2, 1, 3).reshape(G.P, S, G.NH * d), n_heads=7)
    with pytest.raises(ValueError, match="heads"):
        f(q, K, V, n_heads=G.NH + 1)
    with pytest.raises(ValueError):
        f(q, K, V[:, :, :-1])
    with pytest.raises(ValueError):
        f(q, K, V.float())
    with pytest.raises(ValueError):
        f(q.float(), K, V)
    with pytest.raises(ValueError, match="key_mask"):
        f(q, K, V, mask.repeat_interleave(Gn, 0))                    # the mask is per prompt
    with pytest.raises(ValueError, match="key_mask"):
        f(q, K, V, mask.to(torch.int32))
    with pytest.raises(ValueError, match="live"):
        f(q, K, V, mask, live=torch.ones(G.P, dtype=torch.int64))    # live is per row
    with pytest.raises(ValueError):
        f(q, K[0], V[0])                                             # 3-D without n_heads
    with pytest.raises(ValueError):
        f(q, K.reshape(-1), V.reshape(-1))
    with pytest.raises(TypeError):
        f(q, [K], [V])
    # off the device the call does what the existing one does on the expanded operands
    with pytest.raises(ValueError) as mine:
        f(q, K, V, mask)
    with pytest.raises(ValueError) as theirs:
        P.t5_decode_cross_attention(q, G.expand(K, Gn), G.expand(V, Gn), G.expand(mask, Gn))
    assert str(mine.value) == str(theirs.value)
    h = dict(q=q.to(torch.float16), K=K.to(torch.float16), V=V.to(torch.float16))   # a dtype the kernel does not take
    want = P.t5_decode_cross_attention(h["q"], G.expand(h["K"], Gn), G.expand(h["V"], Gn), G.expand(mask, Gn))
    assert C.same(f(h["q"], h["K"], h["V"], mask), want)
    k3 = h["K"].permute(0, 2, 1, 3).reshape(G.P, S, G.NH * d)
    v3 = h["V"].permute(0, 2, 1, 3).reshape(G.P, S, G.NH * d)
    assert C.same(f(h["q"][:, None], k3, v3, mask, n_heads=G.NH), want)
