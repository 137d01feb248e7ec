"""Host-side checks of the T5 decode-step attention (no GPU): the bias table against HF's
compute_bias bit for bit, the float64 oracle of tests/t5_decode_attn_checks.py against the
installed transformers' T5Attention stepped token by token with its own cache, and the header /
binding / argument checks that need no device."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_decode_attn_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_attention(is_decoder_self, seed):
    """A float64 T5Attention on a tiny random config (inner width = d_model, eager attention)."""
    pytest.importorskip("transformers")
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention

    torch.manual_seed(seed)
    cfg = T5Config(vocab_size=32, d_model=24, d_kv=8, num_heads=3, d_ff=32, num_layers=1, num_decoder_layers=1,
                   relative_attention_num_buckets=C.NUM_BUCKETS, relative_attention_max_distance=C.MAX_DISTANCE,
                   dropout_rate=0.0, is_decoder=True)
    if hasattr(cfg, "_attn_implementation"):
        cfg._attn_implementation = "eager"
    kw = {"layer_idx": 0} if "layer_idx" in inspect.signature(T5Attention.__init__).parameters else {}
    att = T5Attention(cfg, has_relative_attention_bias=is_decoder_self, **kw).double().eval()
    for p in att.parameters():
        torch.nn.init.normal_(p, std=0.3)
    return att, cfg


def hf_bias_row(att, t):
    """compute_bias for the single query at position t over keys 0..t, whatever the installed signature."""
    params = inspect.signature(att.compute_bias).parameters
    if "past_seen_tokens" in params:
        return att.compute_bias(1, t + 1, past_seen_tokens=t)
    if "cache_position" in params:
        return att.compute_bias(1, t + 1, cache_position=torch.tensor([t]))
    return att.compute_bias(t + 1, t + 1)[:, :, -1:, :]


def test_bias_table_equals_hf_compute_bias_bit_for_bit():
    """Every t in 0..299: the exact buckets below 16, the logarithmic ones, the saturation at 128."""
    att, cfg = tiny_attention(True, 0)
    att = att.float()
    w = att.relative_attention_bias.weight
    table = P.t5_relative_bias_table(w, 300, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
    assert table.dtype == torch.float32 and tuple(table.shape) == (cfg.num_heads, 300) and table.is_contiguous()
    with torch.no_grad():
        for t in range(300):
            want = hf_bias_row(att, t)[0, :, 0, :]                       # [nH, t + 1], key j at column j
            got = table[:, :t + 1].flip(1)                               # distance t - j at column j
            assert torch.equal(got, want), t
    # the oracle's Python-float buckets are the same numbers
    buckets = [C.bucket(d) for d in range(300)]
    assert torch.equal(table, w.detach()[torch.tensor(buckets)].t())
    assert buckets[:17] == list(range(17)) and buckets[127] == 31 and buckets[128] == 31 and max(buckets) == 31


def test_bias_table_refuses_a_wrong_weight():
    with pytest.raises(ValueError):
        P.t5_relative_bias_table(torch.zeros(16, 4), 10)
    with pytest.raises(ValueError):
        P.t5_relative_bias_table(torch.zeros(32, 4), 0)


def _cache():
    from transformers import DynamicCache
    try:
        from transformers import EncoderDecoderCache
        return EncoderDecoderCache(DynamicCache(), DynamicCache())
    except ImportError:
        return DynamicCache()


def test_oracle_against_hf_self_attention_with_bias():
    """HF's module stepped token by token with its own cache past the bucket saturation; the oracle
    steps the module's own projections of the same tokens."""
    att, cfg = tiny_attention(True, 1)
    Bt, steps, nH, d = 2, 140, cfg.num_heads, cfg.d_kv
    g = torch.Generator().manual_seed(2)
    hs = torch.randn(Bt, steps, cfg.d_model, generator=g, dtype=torch.float64)
    K = torch.zeros(Bt, nH, steps, d, dtype=torch.float64)
    V = torch.zeros_like(K)
    W = att.relative_attention_bias.weight.detach()
    cache = _cache()
    worst = 0.0
    with torch.no_grad():
        for t in range(steps):
            h = hs[:, t:t + 1]
            want = att(h, past_key_values=cache)[0][:, 0]
            q, k, v = (lin(h)[:, 0].reshape(Bt, nH, d) for lin in (att.q, att.k, att.v))
            got = att.o(C.oracle_self_step(q, k, v, K, V, t, W))
            worst = max(worst, float((got - want).abs().max()))
    assert worst < 1e-12, worst


def test_oracle_against_hf_cross_attention_with_a_holed_mask():
    att, cfg = tiny_attention(False, 3)
    Bt, S, steps, nH, d = 3, 11, 4, cfg.num_heads, cfg.d_kv
    g = torch.Generator().manual_seed(4)
    enc = torch.randn(Bt, S, cfg.d_model, generator=g, dtype=torch.float64)
    mask = C.make_mask("holes", Bt, S, g)
    assert int((mask == 0).sum()) > 0
    add = torch.zeros(Bt, 1, 1, S, dtype=torch.float64).masked_fill((mask == 0)[:, None, None, :],
                                                                    torch.finfo(torch.float64).min)
    cache = _cache()
    with torch.no_grad():
        Ke = att.k(enc).reshape(Bt, S, nH, d).transpose(1, 2)
        Ve = att.v(enc).reshape(Bt, S, nH, d).transpose(1, 2)
        for t in range(steps):
            h = torch.randn(Bt, 1, cfg.d_model, generator=g, dtype=torch.float64)
            want = att(h, mask=add, key_value_states=enc, past_key_values=cache)[0][:, 0]
            q = att.q(h)[:, 0].reshape(Bt, nH, d)
            got = att.o(C.oracle_cross(q, Ke, Ve, mask))
            assert float((got - want).abs().max()) < 1e-12, t


def test_oracle_fully_masked_row_is_zero_and_ignores_masked_rows():
    c = C.cross_case(torch.float32, 64, 9, "holes")
    mask = c["mask"].clone()
    mask[1] = 0
    out = C.oracle_cross(c["q"], C.poison(c["K"], mask), C.poison(c["V"], mask), mask)
    assert torch.isfinite(out).all() and float(out[1].abs().max()) == 0.0 and float(out[0].abs().max()) > 0.0


# ------------------------------------------------------------------ header, binding, host-side refusals
def test_header_declares_and_the_binding_binds_the_entry():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    assert "int trlx_t5_decode_attn(const TrlxT5DecodeAttnArgs* a, void* stream);" in txt
    res, args = _lib.SIGNATURES["trlx_t5_decode_attn"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.T5DecodeAttnArgs), ctypes.c_void_p]
    assert (_lib.T5_ATTN_SELF, _lib.T5_ATTN_CROSS) == (0, 1)
    assert "#define TRLX_T5_ATTN_SELF 0" in txt and "#define TRLX_T5_ATTN_CROSS 1" in txt


def test_struct_mirror_matches_the_header(tmp_path):
    fields = [f[0] for f in _lib.T5DecodeAttnArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(TrlxT5DecodeAttnArgs, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(TrlxT5DecodeAttnArgs));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [getattr(_lib.T5DecodeAttnArgs, f).offset for f in fields] + [ctypes.sizeof(_lib.T5DecodeAttnArgs)]


def _args(**over):
    """A self-attention argument record over host buffers: every refusal below is decided before
    any launch, so nothing dereferences them."""
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    kw = dict(q=p, ldq=5 * 64, k_new=p, ldk=5 * 64, v_new=p, ldv=5 * 64, k=p, v=p, bias_by_distance=None,
              key_mask=None, out=p, B=3, n_heads=5, d_kv=64, max_len=160, t=0, dtype=_lib.BF16,
              mode=_lib.T5_ATTN_SELF)
    kw.update(over)
    a = _lib.T5DecodeAttnArgs(**kw)
    a._keep = buf
    return a


@pytest.mark.parametrize("over,word", [
    (dict(d_kv=96), "d_kv"), (dict(d_kv=32), "d_kv"), (dict(dtype=_lib.I64), "dtype"), (dict(t=160), "t 160"),
    (dict(t=-1), "t -1"), (dict(ldq=5 * 64 - 8), "q row stride"), (dict(ldk=8), "row strides"),
    (dict(ldv=5 * 64 + 4), "row strides"), (dict(q=None), "NULL"), (dict(out=None), "NULL"),
    (dict(k_new=None), "k_new"), (dict(key_mask=1 << 12), "key_mask"), (dict(mode=2), "mode"),
    (dict(mode=_lib.T5_ATTN_CROSS), "self-attention only"), (dict(B=0), "B 0"), (dict(max_len=0), "max_len 0"),
])
def test_entry_refuses_bad_arguments_before_any_launch(over, word):
    with pytest.raises(ValueError, match="status 5") as e:
        _lib.call("trlx_t5_decode_attn", ctypes.byref(_args(**over)), None)
    assert word in str(e.value)


def test_entry_refuses_a_misaligned_pointer():
    a = _args()
    a.q = a.q + 2
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.call("trlx_t5_decode_attn", ctypes.byref(a), None)


def test_python_entries_check_before_touching_the_device():
    cache = P.T5DecodeKVCache(2, 3, 64, 5, torch.float32, "cpu")
    x = torch.zeros(2, 3 * 64)
    with pytest.raises(ValueError, match="outside"):
        P.t5_decode_self_attention(x, x, x, cache, 5)
    with pytest.raises(ValueError, match="ROCm"):
        P.t5_decode_self_attention(x, x, x, cache, 0)
    with pytest.raises(ValueError, match="bias_table"):
        P.t5_decode_self_attention(x, x, x, cache, 0, bias_table=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="key_mask"):
        P.t5_decode_cross_attention(x, cache.k, cache.v, key_mask=torch.ones(2, 5, dtype=torch.int32))


def test_other_widths_run_the_torch_expression():
    """d_kv outside {64, 128}: the documented torch route, equal to the oracle (here on the CPU)."""
    g = torch.Generator().manual_seed(5)
    Bt, nH, d, L = 2, 3, 16, 6
    cache = P.T5DecodeKVCache(Bt, nH, d, L, torch.float32, "cpu")
    W = torch.randn(32, nH, generator=g)
    table = P.t5_relative_bias_table(W, L)
    K = torch.zeros(Bt, nH, L, d, dtype=torch.float64)
    V = torch.zeros_like(K)
    for t in range(L):
        q, k, v = (torch.randn(Bt, nH, d, generator=g) for _ in range(3))
        got = P.t5_decode_self_attention(q, k, v, cache, t, table)
        want = C.oracle_self_step(q, k, v, K, V, t, W)
        assert C.max_err(got, want) < 1e-5
    mask = C.make_mask("holes", Bt, L, g)
    mask[1] = 0
    got = P.t5_decode_cross_attention(q, cache.k, cache.v, mask)
    assert C.max_err(got, C.oracle_cross(q, cache.k, cache.v, mask)) < 1e-5 and float(got[1].abs().max()) == 0.0
