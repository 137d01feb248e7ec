"""Host-side checks of T5's full-sequence attention (no GPU): the offset bias table against HF's
compute_bias bit for bit, the float64 oracle of tests/t5_attention_checks.py against the installed
transformers' T5Attention in its three uses, that the GPU test's rule tells a wrong bias index, a
dropped key and an off-by-one causal boundary from a right result, the torch fallback, and the
header / binding / argument checks that need no device."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_attention_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_attention(is_decoder, has_bias, seed, dtype=torch.float64):
    pytest.importorskip("transformers")
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention

    torch.manual_seed(seed)
    cfg = T5Config(vocab_size=32, d_model=24, d_kv=8, num_heads=3, d_ff=32, num_layers=1, num_decoder_layers=1,
                   relative_attention_num_buckets=C.NUM_BUCKETS, relative_attention_max_distance=C.MAX_DISTANCE,
                   dropout_rate=0.0, is_decoder=is_decoder)
    if hasattr(cfg, "_attn_implementation"):
        cfg._attn_implementation = "eager"
    kw = {"layer_idx": 0} if "layer_idx" in inspect.signature(T5Attention.__init__).parameters else {}
    att = T5Attention(cfg, has_relative_attention_bias=has_bias, **kw).to(dtype).eval()
    for p in att.parameters():
        torch.nn.init.normal_(p, std=0.3)
    return att, cfg


def heads(x, nH, d):
    return x.reshape(x.shape[0], x.shape[1], nH, d).transpose(1, 2)


# ------------------------------------------------------------------ the bias table
@pytest.mark.parametrize("bidirectional,Tq,S", [(True, 1, 1), (True, 17, 17), (True, 200, 200), (True, 48, 300),
                                                (False, 130, 130)])
def test_bias_offsets_equal_hf_compute_bias_bit_for_bit(bidirectional, Tq, S):
    """Every (i, j): both signs, the exact buckets, the logarithmic ones, the saturation at 128."""
    att, cfg = tiny_attention(not bidirectional, True, 0, torch.float32)
    w = att.relative_attention_bias.weight
    table = P.t5_relative_bias_offsets(w, Tq, S, bidirectional, cfg.relative_attention_num_buckets,
                                       cfg.relative_attention_max_distance)
    assert table.dtype == torch.float32 and tuple(table.shape) == (cfg.num_heads, Tq + S - 1) and table.is_contiguous()
    with torch.no_grad():
        want = att.compute_bias(Tq, S)[0]                                                  # [nH, Tq, S]
    rel = torch.arange(S)[None, :] - torch.arange(Tq)[:, None]
    assert torch.equal(table[:, rel + (Tq - 1)], want)
    # the oracle's Python-float buckets are the same numbers
    assert torch.equal(C.oracle_bias(w.detach(), Tq, S, bidirectional).float(), want)
    if Tq >= 130:   # distances on both sides of the exact / log boundary and of the saturation
        half = C.NUM_BUCKETS // 2 if bidirectional else C.NUM_BUCKETS
        got = [C.bucket(-x, bidirectional) for x in (half // 2 - 1, half // 2, 127, 128, 129)]
        assert got[0] == half // 2 - 1 and got[1] == half // 2 and got[3] == got[4] == half - 1
        if bidirectional:
            assert [C.bucket(x, True) for x in (7, 8, 128, 129)] == [half + 7, half + 8, 2 * half - 1, 2 * half - 1]


def test_bias_offsets_refuse_a_wrong_weight():
    with pytest.raises(ValueError):
        P.t5_relative_bias_offsets(torch.zeros(16, 4), 10, 10, True)
    with pytest.raises(ValueError):
        P.t5_relative_bias_offsets(torch.zeros(32, 4), 0, 10, True)


# ------------------------------------------------------------------ the oracle against transformers
def test_oracle_against_hf_encoder_self_attention_left_padded():
    att, cfg = tiny_attention(False, True, 1)
    Bt, T, nH, d = 3, 150, cfg.num_heads, cfg.d_kv
    g = torch.Generator().manual_seed(2)
    hs = torch.randn(Bt, T, cfg.d_model, generator=g, dtype=torch.float64)
    mask = C.make_mask("left", Bt, T, g)
    assert int((mask == 0).sum()) > 0 and int(mask.sum(1).min()) >= 1
    add = torch.zeros(Bt, 1, 1, T, dtype=torch.float64).masked_fill((mask == 0)[:, None, None, :],
                                                                    torch.finfo(torch.float64).min)
    with torch.no_grad():
        want = att(hs, mask=add)[0]
        q, k, v = (heads(lin(hs), nH, d) for lin in (att.q, att.k, att.v))
        got = att.o(C.oracle(q, k, v, att.relative_attention_bias.weight.detach(), True, mask=mask))
    assert float((got - want).abs().max()) < 1e-12


def test_oracle_against_hf_decoder_self_attention_teacher_forced():
    att, cfg = tiny_attention(True, True, 3)
    Bt, T, nH, d = 2, 140, cfg.num_heads, cfg.d_kv
    g = torch.Generator().manual_seed(4)
    hs = torch.randn(Bt, T, cfg.d_model, generator=g, dtype=torch.float64)
    causal = torch.zeros(T, T, dtype=torch.float64).masked_fill(torch.ones(T, T).triu(1).bool(),
                                                                torch.finfo(torch.float64).min)
    with torch.no_grad():
        want = att(hs, mask=causal[None, None])[0]
        q, k, v = (heads(lin(hs), nH, d) for lin in (att.q, att.k, att.v))
        got = att.o(C.oracle(q, k, v, att.relative_attention_bias.weight.detach(), False, causal=True))
    assert float((got - want).abs().max()) < 1e-12


def test_oracle_against_hf_cross_attention_with_a_holed_mask():
    att, cfg = tiny_attention(True, False, 5)
    Bt, Tq, S, nH, d = 3, 7, 21, cfg.num_heads, cfg.d_kv
    g = torch.Generator().manual_seed(6)
    hs = torch.randn(Bt, Tq, cfg.d_model, generator=g, dtype=torch.float64)
    enc = torch.randn(Bt, S, cfg.d_model, generator=g, dtype=torch.float64)
    mask = C.make_mask("holes", Bt, S, g)
    add = torch.zeros(Bt, 1, 1, S, dtype=torch.float64).masked_fill((mask == 0)[:, None, None, :],
                                                                    torch.finfo(torch.float64).min)
    with torch.no_grad():
        want = att(hs, mask=add, key_value_states=enc)[0]
        q = heads(att.q(hs), nH, d)
        k, v = heads(att.k(enc), nH, d), heads(att.v(enc), nH, d)
        got = att.o(C.oracle(q, k, v, mask=mask))
    assert float((got - want).abs().max()) < 1e-12


def test_oracle_fully_masked_row_is_zero_and_ignores_masked_rows():
    c = C.case(64, 5, 9, "holes")
    mask = c["mask"].clone()
    mask[1] = 0
    out = C.oracle(c["q"], C.poison(c["k"], mask), C.poison(c["v"], mask), c["W"], True, mask=mask)
    assert torch.isfinite(out).all() and float(out[1].abs().max()) == 0.0 and float(out[0].abs().max()) > 0.0


# ------------------------------------------------------------------ the rule discriminates
def test_the_rule_tells_wrong_results_from_right_ones():
    """The bound the bf16 eager route's own (CPU) error yields, against three wrong oracles: each is
    more than 10x outside it."""
    d, T = 64, 24
    c = C.case(d, T, T, "right", seed=1)
    mask = c["mask"]
    table = P.t5_relative_bias_offsets(c["W"], T, T, True)
    want = C.oracle(c["q"], c["k"], c["v"], c["W"], True, mask=mask)
    lim = C.bound(C.max_err(C.eager(c["q"], c["k"], c["v"], table, mask), want), want)
    live = (int(mask[0].nonzero()[0]), int(mask[1].nonzero()[-1]))
    shifted = C.oracle(c["q"], c["k"], c["v"], c["W"], True, mask=mask, bias_shift=1)
    dropped = [C.oracle(c["q"], c["k"], c["v"], c["W"], True, mask=mask, drop_key=(b, live[b])) for b in (0, 1)]
    assert C.max_err(shifted, want) > 10 * lim, (C.max_err(shifted, want), lim)
    for b in (0, 1):
        assert C.max_err(dropped[b][b], want[b]) > 10 * lim, (b, C.max_err(dropped[b][b], want[b]), lim)
    tableu = P.t5_relative_bias_offsets(c["W"], T, T, False)
    wantc = C.oracle(c["q"], c["k"], c["v"], c["W"], False, causal=True)
    limc = C.bound(C.max_err(C.eager(c["q"], c["k"], c["v"], tableu, None, True), wantc), wantc)
    for shift in (-1, 1):
        off = C.oracle(c["q"], c["k"], c["v"], c["W"], False, causal=True, causal_shift=shift)
        assert C.max_err(off, wantc) > 10 * limc, (shift, C.max_err(off, wantc), limc)


# ------------------------------------------------------------------ the torch fallback
@pytest.mark.parametrize("mode", ["encoder", "decoder", "cross"])
def test_other_dtypes_and_widths_run_the_torch_expression(mode):
    """fp32, d_kv 32: the documented torch route, equal to the oracle (here on the CPU), in all
    three operand forms."""
    Tq, S = (9, 9) if mode != "cross" else (5, 12)
    c = C.case(32, Tq, S, "holes" if mode != "decoder" else "none", dtype=torch.float32)
    mask = c["mask"].clone() if c["mask"] is not None else None
    if mask is not None:
        mask[1] = 0                                               # a fully masked row: zeros
    kw = dict(key_mask=mask)
    okw = dict(mask=mask)
    if mode != "cross":
        kw["bias"] = P.t5_relative_bias_offsets(c["W"], Tq, S, mode == "encoder")
        okw.update(weight=c["W"], bidirectional=mode == "encoder")
    if mode == "decoder":
        kw["causal"] = okw["causal"] = True
    want = C.oracle(c["q"], c["k"], c["v"], **okw)
    k, v = C.poison(c["k"], mask), C.poison(c["v"], mask)
    got = P.t5_attention(c["q"], k, v, **kw)
    assert tuple(got.shape) == (C.B, Tq, C.NH * 32) and got.dtype == torch.float32
    assert C.max_err(got, want) < 1e-5
    if mask is not None:
        assert float(got[1].abs().max()) == 0.0
    bthd = [x.transpose(1, 2).contiguous() for x in (c["q"], k, v)]
    assert torch.equal(P.t5_attention(*bthd, layout="bthd", **kw), got)
    flat = [x.flatten(2) for x in bthd]
    assert torch.equal(P.t5_attention(*flat, n_heads=C.NH, **kw), got)


# ------------------------------------------------------------------ refusals
def test_python_entry_refusals():
    q = torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 3, 7, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="causal"):
        P.t5_attention(q, k, k, causal=True)
    with pytest.raises(ValueError, match="key_mask"):
        P.t5_attention(q, k, k, key_mask=torch.ones(2, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="key_mask"):
        P.t5_attention(q, k, k, key_mask=torch.ones(2, 6, dtype=torch.int64))
    with pytest.raises(ValueError, match="bias"):
        P.t5_attention(q, k, k, bias=torch.zeros(3, 5 + 7))
    with pytest.raises(ValueError, match="bias"):
        P.t5_attention(q, k, k, bias=torch.zeros(3, 5 + 7 - 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="disagree"):
        P.t5_attention(q, k, k[:, :2])
    with pytest.raises(ValueError, match="n_heads"):
        P.t5_attention(q.flatten(2), k, k)
    with pytest.raises(ValueError, match="ROCm"):
        P.t5_attention(q, k, k)
    qg = q.clone().requires_grad_()
    with pytest.raises(RuntimeError, match="torch_fallback"):
        P.t5_attention(qg, k, k)
    with torch.no_grad():
        with pytest.raises(ValueError, match="ROCm"):   # no_grad: past the autograd check
            P.t5_attention(qg, k, k)


def test_tiles_are_exported():
    from trlx_t5_amd import t5_attention as mod_or_fn
    assert P.t5_attention.Q_TILE == mod_or_fn.Q_TILE >= 32 and P.t5_attention.KV_TILE == mod_or_fn.KV_TILE >= 16
    q_tile, kv_tile = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("trlx_t5_attention_tiles", ctypes.byref(q_tile), ctypes.byref(kv_tile))
    assert (q_tile.value, kv_tile.value) == (P.t5_attention.Q_TILE, P.t5_attention.KV_TILE)


# ------------------------------------------------------------------ header, binding, the C entry's refusals
def test_header_declares_and_the_binding_binds_the_entry():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    assert "int trlx_t5_attention(const TrlxT5AttentionArgs* a, void* stream);" in txt
    res, args = _lib.SIGNATURES["trlx_t5_attention"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.T5AttentionArgs), ctypes.c_void_p]


def test_struct_mirror_matches_the_header(tmp_path):
    fields = [f[0] for f in _lib.T5AttentionArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(TrlxT5AttentionArgs, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(TrlxT5AttentionArgs));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [getattr(_lib.T5AttentionArgs, f).offset for f in fields] + [ctypes.sizeof(_lib.T5AttentionArgs)]


def c_args(**over):
    """An argument record over a host buffer, B 2, Tq = S = 5, nH 3, d_kv 64, [B, T, nH*d] operands:
    every refusal below is decided before any launch, so nothing dereferences it."""
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    nH, d, T = 3, 64, 5
    kw = dict(B=2, n_heads=nH, d_kv=d, Tq=T, S=T, dtype=_lib.BF16, causal=0, bias_by_offset=None, key_mask=None)
    for n in ("q", "k", "v", "o"):
        kw["out" if n == "o" else n] = p
        kw[f"{n}_stride_b"], kw[f"{n}_stride_t"], kw[f"{n}_stride_h"] = T * nH * d, nH * d, d
    kw.update(over)
    a = _lib.T5AttentionArgs(**kw)
    a._keep = buf
    return a


@pytest.mark.parametrize("over,word", [
    (dict(dtype=_lib.F32), "dtype"), (dict(dtype=_lib.I64), "dtype"), (dict(d_kv=96), "d_kv"), (dict(d_kv=32), "d_kv"),
    (dict(causal=1, S=6), "causal"), (dict(q=None), "NULL"), (dict(out=None), "NULL"),
    (dict(q_stride_t=3 * 64 + 4), "q strides"), (dict(k_stride_h=32), "k strides"), (dict(v_stride_b=-960), "v strides"),
    (dict(o_stride_t=64), "out strides"), (dict(o_stride_b=3 * 64), "out strides"), (dict(B=0), "B 0"),
    (dict(Tq=0), "Tq 0"), (dict(S=(1 << 30) + 1), "S 1073741825"), (dict(B=1 << 30, n_heads=1 << 10), "grid"),
    (dict(k_stride_t=1 << 62, S=1 << 20), "k strides"), (dict(key_mask=(1 << 12) + 4), "key_mask"),
    (dict(bias_by_offset=(1 << 12) + 2), "bias_by_offset"),
])
def test_entry_refuses_bad_arguments_before_any_launch(over, word):
    with pytest.raises(ValueError, match="status 5") as e:
        _lib.call("trlx_t5_attention", ctypes.byref(c_args(**over)), None)
    assert word in str(e.value)


def test_entry_refuses_a_misaligned_pointer():
    a = c_args()
    a.k = a.k + 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.call("trlx_t5_attention", ctypes.byref(a), None)
