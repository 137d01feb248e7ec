"""Host-side checks of the T5 feed-forward activation (no GPU): the float64 oracle against HF's own
modules, T5FeedForward in float64 against them end to end, that the GPU test's rule takes a
single-rounding fp32 restatement of the kernel and refuses four wrong ones, the state_dict names,
the argument errors, and the header / binding checks that need no device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
from transformers import T5Config
from transformers.models.t5.modeling_t5 import T5DenseActDense, T5DenseGatedActDense

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_ff_act_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# feed_forward_proj -> (HF class, the activation it maps to, gated)
FORMS = {"gated-gelu": (T5DenseGatedActDense, "gelu_new", True), "gated-silu": (T5DenseGatedActDense, "silu", True),
         "relu": (T5DenseActDense, "relu", False)}


def _config(proj, d_model=24, d_ff=40):
    return T5Config(d_model=d_model, d_ff=d_ff, feed_forward_proj=proj, dropout_rate=0.0)


def _hf(proj, seed=0):
    torch.manual_seed(seed)
    cfg = _config(proj)
    return cfg, FORMS[proj][0](cfg).double().eval()


# ------------------------------------------------------------------ the oracle is HF's module
@pytest.mark.parametrize("proj", list(FORMS))
def test_the_oracle_forward_is_the_hf_module_activation(proj):
    cfg, hf = _hf(proj)
    _, act, gated = FORMS[proj]
    assert (cfg.dense_act_fn, cfg.is_gated_act) == (act, gated)
    c = C.case(9, 40, torch.float32, scale=3.0, gated=gated, tail=False)
    u = c["u"].double()
    want = hf.act(u) if not gated else hf.act(u) * c["v"].double()
    got = C.oracle(c["u"], c["v"], c["dy"], act)["y"]
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("proj", list(FORMS))
def test_feed_forward_in_float64_is_the_hf_module(proj):
    cfg, hf = _hf(proj)
    m = P.T5FeedForward(cfg).double()
    m.load_state_dict(hf.state_dict(), strict=True)
    x = torch.randn(3, 5, cfg.d_model, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    x1, x2 = x.clone().requires_grad_(), x.clone().requires_grad_()
    y1, y2 = m(x1), hf(x2)
    assert float((y1 - y2).detach().abs().max()) <= 1e-12 * float(y2.detach().abs().max())
    g = torch.randn(y2.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y1.backward(g)
    y2.backward(g)
    assert float((x1.grad - x2.grad).abs().max()) <= 1e-12 * float(x2.grad.abs().max())
    for (n1, p1), (n2, p2) in zip(sorted(m.named_parameters()), sorted(hf.named_parameters())):
        assert n1 == n2
        assert float((p1.grad - p2.grad).abs().max()) <= 1e-12 * float(p2.grad.abs().max()), n1


def test_packed_in_float64_is_the_separate_call():
    c = C.case(5, 12, torch.float32, tail=False)
    uv = torch.cat([c["u"], c["v"]], dim=-1).double().requires_grad_()
    u, v = c["u"].double().requires_grad_(), c["v"].double().requires_grad_()
    for act in C.ACTS:
        y1, y2 = P.t5_ff_act_packed(uv, act), P.t5_ff_act(u, v, act)
        assert torch.equal(y1, y2)
        (g1,) = torch.autograd.grad(y1, [uv], c["dy"].double())
        gu, gv = torch.autograd.grad(y2, [u, v], c["dy"].double())
        assert g1.shape == uv.shape and torch.equal(g1, torch.cat([gu, gv], dim=-1))


# ------------------------------------------------------------------ state_dict
@pytest.mark.parametrize("proj", list(FORMS))
def test_state_dict_names_and_strict_load_both_ways(proj):
    cfg, hf = _hf(proj)
    m = P.T5FeedForward(cfg)
    want = ["wi_0.weight", "wi_1.weight", "wo.weight"] if FORMS[proj][2] else ["wi.weight", "wo.weight"]
    assert sorted(m.state_dict()) == want == sorted(hf.state_dict())
    m.double().load_state_dict(hf.state_dict(), strict=True)
    torch.manual_seed(5)
    other = FORMS[proj][0](cfg).double()
    other.load_state_dict(m.state_dict(), strict=True)
    for n, p in other.state_dict().items():
        assert torch.equal(p, hf.state_dict()[n])
    assert not any(isinstance(x, torch.nn.Dropout) for x in m.modules())


# ------------------------------------------------------------------ the rule
def _rule_inputs(dtype, act, gated):
    """N(0, 1) * {1, 3} with the tail row, as the GPU test draws them."""
    for scale in (1.0, 3.0):
        yield C.case(6, 515, dtype, scale=scale, gated=gated, seed=int(scale))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("gated", [True, False], ids=["gated", "ungated"])
@pytest.mark.parametrize("act", C.ACTS)
def test_a_single_rounding_fp32_restatement_is_inside_the_rule(act, gated, dtype):
    for c in _rule_inputs(dtype, act, gated):
        want = C.oracle(c["u"], c["v"], c["dy"], act)
        got = C.restated(c["u"], c["v"], c["dy"], act)
        figs = C.judge(got, want, c["u"], c["v"], c["dy"], dtype)
        print(act, gated, dtype, figs)
        assert set(figs) == ({"y", "du", "dv"} if gated else {"y", "du"})
        for n, r in figs.items():
            assert r <= 1.0, (n, figs)
            assert bool(torch.isfinite(got[n]).all()), n
            if dtype == torch.bfloat16:
                assert r <= 0.51, (n, figs)      # half an ulp of the one rounding, fp32 error on top


WRONG = {"erf": ("y", "du", "dv"), "silu": ("y", "du", "dv"), "swapped": ("y", "du", "dv"), "no_cubic": ("du",)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(WRONG))
def test_the_rule_refuses_a_wrong_variant(name, dtype):
    """Each wrong gelu_new, evaluated in float64 and rounded once as a kernel's result would be, is
    outside the rule in every output it must disturb."""
    worst = {n: 0.0 for n in WRONG[name]}
    for c in _rule_inputs(dtype, "gelu_new", True):
        want = C.oracle(c["u"], c["v"], c["dy"], "gelu_new")
        got = C.restated(c["u"], c["v"], c["dy"], "gelu_new", wrong=name)
        figs = C.judge(got, want, c["u"], c["v"], c["dy"], dtype)
        for n in worst:
            worst[n] = max(worst[n], figs[n])
    print(name, dtype, worst)
    for n, r in worst.items():
        assert r > 1.0, (name, n, worst)


def test_hf_eager_bf16_is_outside_the_rule_and_recorded():
    """Not a yardstick, a figure: HF's op sequence rounds every op to bf16."""
    worst = 0.0
    for scale in (1.0, 3.0):                    # no tail row: HF's own backward gives 0 * inf there
        c = C.case(6, 515, torch.bfloat16, scale=scale, seed=int(scale), tail=False)
        u, v, dy = c["u"], c["v"], c["dy"]
        want = C.oracle(u, v, dy, "gelu_new")
        figs = C.judge(C.eager(u, v, dy, "gelu_new"), want, u, v, dy, torch.bfloat16)
        worst = max(worst, *figs.values())
    print("HF eager bf16 gelu_new, worst ratio to the rule:", worst)
    assert worst > 10.0


def test_ulp_is_the_spacing_of_the_format():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 3e38, 1e-30, 0.0], dtype=torch.float64)
    for dtype in (torch.bfloat16, torch.float32):
        got = C.ulp(x, dtype)
        xr = x.to(dtype)
        up = torch.nextafter(xr.float(), torch.tensor(float("inf"))).double() if dtype == torch.float32 else None
        assert float(got[-1]) == 0.0
        if up is not None:
            assert torch.equal(got[:-1], (up - xr.double())[:-1])
    assert float(C.ulp(torch.tensor([1.0], dtype=torch.float64), torch.bfloat16)) == 2.0 ** -7
    assert float(C.ulp(torch.tensor([-3.9], dtype=torch.float64), torch.bfloat16)) == 2.0 ** -6


# ------------------------------------------------------------------ argument errors, before the library is needed
def test_argument_errors(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", no_library)
    monkeypatch.setattr(_lib, "load", no_library)
    u = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="act must be"):
        P.t5_ff_act(u, u, act="gelu")
    with pytest.raises(ValueError, match="act must be"):
        P.t5_ff_act_packed(u, act="tanh")
    with pytest.raises(ValueError, match="share shape, dtype and device"):
        P.t5_ff_act(u, u[:, :2])
    with pytest.raises(ValueError, match="share shape, dtype and device"):
        P.t5_ff_act(u, u.to(torch.bfloat16))
    with pytest.raises(ValueError, match=r"\[\.\.\., 2F\]"):
        P.t5_ff_act_packed(torch.zeros(2, 7))
    with pytest.raises(ValueError, match=r"\[\.\.\., F\]"):
        P.t5_ff_act(torch.zeros(()))
    with pytest.raises(TypeError):
        P.t5_ff_act([1.0, 2.0])
    with pytest.raises(ValueError, match="no CPU path"):        # kernel dtypes off the device: as t5_attention
        P.t5_ff_act(u, u)
    with pytest.raises(ValueError, match="act must be"):        # an activation the kernel lacks: at construction
        P.T5FeedForward(T5Config(d_model=8, d_ff=16, feed_forward_proj="gelu"))
    with pytest.raises(ValueError, match="act must be"):
        P.T5FeedForward(T5Config(d_model=8, d_ff=16, feed_forward_proj="gated-tanh"))


def test_other_dtypes_take_the_torch_expression():
    c = C.case(3, 10, torch.float32, tail=False)
    for dt in (torch.float64, torch.float16):
        u, v = c["u"].to(dt), c["v"].to(dt)
        for act in C.ACTS:
            assert torch.equal(P.t5_ff_act(u, v, act), C.eager_act(u, act) * v)
            assert torch.equal(P.t5_ff_act(u, None, act), C.eager_act(u, act))


# ------------------------------------------------------------------ header, binding, geometry
ENTRIES = {
    "trlx_t5_ff_act_fwd": "int trlx_t5_ff_act_fwd(const TrlxT5FfActArgs* a, void* stream);",
    "trlx_t5_ff_act_bwd": "int trlx_t5_ff_act_bwd(const TrlxT5FfActArgs* a, void* stream);",
    "trlx_t5_ff_act_geometry":
        "int trlx_t5_ff_act_geometry(int* vec_bf16, int* vec_f32, int* cols_per_block, int* rows_per_block);",
}


def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", txt) and _lib.ABI_VERSION == 2
    for name, decl in ENTRIES.items():
        assert decl in txt, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == len(decl[decl.index("(") + 1:decl.rindex(")")].split(",")), name
    for name in ("trlx_t5_ff_act_fwd", "trlx_t5_ff_act_bwd"):
        assert _lib.SIGNATURES[name][1] == [ctypes.POINTER(_lib.T5FfActArgs), ctypes.c_void_p]
    for name, code in (("RELU", _lib.T5_ACT_RELU), ("GELU_NEW", _lib.T5_ACT_GELU_NEW), ("SILU", _lib.T5_ACT_SILU)):
        assert re.search(rf"TRLX_T5_ACT_{name} = {code},", txt)
    assert {"t5_ff_act", "t5_ff_act_packed", "T5FeedForward"} <= set(P.__all__)


def test_struct_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in _lib.T5FfActArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(TrlxT5FfActArgs, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(TrlxT5FfActArgs));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(_lib.T5FfActArgs, f).offset for f in fields] + [ctypes.sizeof(_lib.T5FfActArgs)]


def test_geometry_and_refusals_need_no_device():
    t = [ctypes.c_int(0) for _ in range(4)]
    _lib.call("trlx_t5_ff_act_geometry", *[ctypes.byref(x) for x in t])
    assert [x.value for x in t] == [P.t5_ff.VEC_BF16, P.t5_ff.VEC_F32, P.t5_ff.COLS_PER_BLOCK, P.t5_ff.ROWS_PER_BLOCK]
    assert P.t5_ff.COLS_PER_BLOCK % (64 * P.t5_ff.VEC_BF16) == 0
    # refused before any launch: these never touch the (fake, aligned) pointers
    base = dict(u=4096, ld_u=8, v=8192, ld_v=8, out=12288, ld_out=8, N=2, F=8, dtype=_lib.BF16, act=_lib.T5_ACT_SILU)
    for entry, bad in (("trlx_t5_ff_act_fwd", dict(u=None)), ("trlx_t5_ff_act_fwd", dict(F=0)),
                       ("trlx_t5_ff_act_fwd", dict(N=-1)), ("trlx_t5_ff_act_fwd", dict(ld_out=7)),
                       ("trlx_t5_ff_act_fwd", dict(dtype=_lib.I64)), ("trlx_t5_ff_act_fwd", dict(act=3)),
                       ("trlx_t5_ff_act_fwd", dict(out=4096 + 2)), ("trlx_t5_ff_act_bwd", dict(dy=None, du=12288)),
                       ("trlx_t5_ff_act_bwd", dict(dy=16384)),
                       ("trlx_t5_ff_act_bwd", dict(dy=16384, v=None, dv=12288, ld_dv=8))):
        with pytest.raises(ValueError):
            _lib.call(entry, ctypes.byref(_lib.T5FfActArgs(**{**base, **bad})), None)
    assert _lib.call("trlx_t5_ff_act_fwd", ctypes.byref(_lib.T5FfActArgs(**{**base, "N": 0})), None) == 0
