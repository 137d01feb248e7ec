"""Host-side checks of the T5 RMSNorm with residual add (no GPU): the float64 oracle against HF's own
T5LayerNorm, that the GPU test's rule takes a single-rounding fp32 restatement of the kernel and
refuses five wrong ones (the sixth is told apart in bits), the module's state_dict, the torch route
of the dtypes the kernel lacks, the argument errors, and the header / binding checks that need no
device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_rmsnorm_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 1), (5, 7), (9, 96), (8, 768), (9, 4096), (2051, 96)]
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


# ------------------------------------------------------------------ the oracle is HF's module
def test_the_oracle_is_the_hf_module():
    hf_t5 = pytest.importorskip("transformers.models.t5.modeling_t5")
    c = C.case(9, 96, torch.float32)
    h = C.rounded_sum(c)
    for dt, tol in ((torch.float64, 2e-6), (torch.float32, 2e-6)):   # HF takes the variance in fp32 in both
        m = hf_t5.T5LayerNorm(96, eps=C.EPS).to(dt)
        with torch.no_grad():
            m.weight.copy_(c["w"])
        want = m(h.to(dt)).detach().double()
        got = C.oracle(h, c["w"], c["dy"])["y"]
        assert float((got - want).abs().max()) <= tol * float(want.abs().max())
    # gradients: the module in float64, on rows whose fp32 variance is exact enough (no 1e-3 rows)
    c = C.case(9, 96, torch.float32, special=False)
    h = C.rounded_sum(c)
    m = hf_t5.T5LayerNorm(96, eps=C.EPS).double()
    with torch.no_grad():
        m.weight.copy_(c["w"])
    hl = h.double().requires_grad_()
    dh, dw = torch.autograd.grad(m(hl), [hl, m.weight], c["dy"].double())
    o = C.oracle(h, c["w"], c["dy"])
    assert float((o["dh"] - dh).abs().max()) <= 2e-6 * float(dh.abs().max())
    assert float((o["dw"] - dw).abs().max()) <= 2e-6 * float(dw.abs().max())
    # the checks' own copy of HF's forward is the module's, bit for bit
    mb = hf_t5.T5LayerNorm(96, eps=C.EPS).to(torch.bfloat16)
    with torch.no_grad():
        mb.weight.copy_(c["w"])
    hb = h.to(torch.bfloat16)
    assert torch.equal(C.hf_norm(hb, mb.weight.detach()), mb(hb).detach())


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
def test_a_single_rounding_fp32_restatement_is_inside_the_rule(dtype):
    for N, D in SHAPES:
        c = C.case(N, D, dtype)
        h = C.rounded_sum(c)
        for with_in in (True, False):
            din = c["dh_in"] if with_in else None
            want = C.oracle(h, c["w"], c["dy"], din)
            got = C.restated(c, dh_in=with_in)
            figs = C.judge(got, want, C.factors(h, c["w"], c["dy"], din), dtype)
            print(N, D, dtype, with_in, figs)
            assert set(figs) == set(C.OUTPUTS)
            for n, r in figs.items():
                assert r <= 1.0, (N, D, n, figs)
                assert bool(torch.isfinite(got[n]).all()), n
                if dtype == torch.bfloat16:
                    assert r <= 0.51, (N, D, n, figs)    # half an ulp of the one rounding, fp32 error on top


DISTURBS = {"layernorm": ("y", "dh", "dw"), "eps_outside": ("y", "dh", "dw"), "dh_no_w": ("dh",),
            "dh_no_projection": ("dh",), "dw_no_rstd": ("dw",)}


@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("name", list(DISTURBS))
def test_the_rule_refuses_a_wrong_variant(name, dtype):
    """Each wrong norm, evaluated in float64 and rounded once as a kernel's result would be, is outside
    the rule in every output it must disturb -- at D = 4096 too, where a mean-subtracting norm would be
    nearly invisible on zero-mean rows."""
    for N, D in ((9, 96), (9, 4096)):
        c = C.case(N, D, dtype)
        h = C.rounded_sum(c)
        want = C.oracle(h, c["w"], c["dy"], c["dh_in"])
        figs = C.judge(C.restated(c, wrong=name), want, C.factors(h, c["w"], c["dy"], c["dh_in"]), dtype)
        print(name, dtype, N, D, figs)
        for n in DISTURBS[name]:
            assert figs[n] > 1.0, (name, n, figs)
        for n in set(C.OUTPUTS) - set(DISTURBS[name]):
            assert figs[n] <= 1.0, (name, n, figs)


def test_the_unrounded_sum_is_told_apart_in_bits():
    """(vi): a norm taken from the fp32 sum before it is rounded to bf16 passes the rule's tolerance
    here and there, so the add form is pinned in bits: its y is the y of the norm of torch's sum."""
    c = C.case(9, 96, torch.bfloat16)
    h = C.rounded_sum(c)
    alone = dict(c, residual=h, x=torch.zeros_like(h))           # the norm of the rounded sum
    good, bad = C.restated(c), C.restated(c, wrong="unrounded_sum")
    assert torch.equal(good["h"], h)
    assert torch.equal(good["y"], C.restated(alone)["y"]) and torch.equal(good["dh"], C.restated(alone)["dh"])
    assert not torch.equal(bad["y"], C.restated(alone)["y"])


def test_hf_eager_bf16_against_the_rule_is_recorded():
    """Not a yardstick, a figure: HF's op sequence rounds h * rstd and then weight * (...)."""
    worst = {n: 0.0 for n in C.OUTPUTS}
    for N, D in ((9, 96), (8, 768)):
        c = C.case(N, D, torch.bfloat16)
        h = C.rounded_sum(c)
        want = C.oracle(h, c["w"], c["dy"], c["dh_in"])
        figs = C.judge(C.eager(h, c["w"], c["dy"], c["dh_in"]), want, C.factors(h, c["w"], c["dy"], c["dh_in"]), torch.bfloat16)
        worst = {n: max(worst[n], figs[n]) for n in worst}
    print("HF eager bf16 T5LayerNorm, worst ratio to the rule:", worst)


# ------------------------------------------------------------------ public surface
ENTRIES = {
    "trlx_t5_rmsnorm_fwd": "int trlx_t5_rmsnorm_fwd(const TrlxT5RmsNormArgs* a, void* stream);",
    "trlx_t5_rmsnorm_bwd": "int trlx_t5_rmsnorm_bwd(const TrlxT5RmsNormArgs* a, void* stream);",
    "trlx_t5_rmsnorm_geometry": "int trlx_t5_rmsnorm_geometry(int64_t N, int64_t D, TrlxT5RmsNormGeometry* g);",
}


def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", txt) and _lib.ABI_VERSION == 2
    for name, decl in ENTRIES.items():
        assert decl in txt, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == len(decl[decl.index("(") + 1:decl.rindex(")")].split(",")), name
    for name in ("trlx_t5_rmsnorm_fwd", "trlx_t5_rmsnorm_bwd"):
        assert _lib.SIGNATURES[name][1] == [ctypes.POINTER(_lib.T5RmsNormArgs), ctypes.c_void_p]
    assert {"t5_rmsnorm", "t5_add_rmsnorm", "T5LayerNorm"} <= set(P.__all__)


@pytest.mark.parametrize("struct, mirror", [("TrlxT5RmsNormArgs", "T5RmsNormArgs"), ("TrlxT5RmsNormGeometry", "T5RmsNormGeometry")])
def test_struct_layout_matches_the_header(tmp_path, struct, mirror):
    cls = getattr(_lib, mirror)
    fields = [f[0] for f in cls._fields_]
    txt = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()
    body = txt[txt.index(f"typedef struct {struct} {{"):txt.index(f"}} {struct};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for line in body.split(";")[:-1] for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", line.split("{")[-1].strip())]
    assert declared == fields                                    # the order of the header's struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof({struct}, {f}));\n' for f in fields)
                   + f'printf("%zu\\n", sizeof({struct}));\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(cls, f).offset for f in fields] + [ctypes.sizeof(cls)]


def test_geometry_and_refusals_need_no_device():
    N = P.t5_norm
    g = N.geometry()
    assert (g["vec_bf16"], g["vec_f32"], g["max_d"], g["max_partials"], g["wave_row_max_d"], g["d_breaks"]) == \
        (N.VEC_BF16, N.VEC_F32, N.MAX_D, N.MAX_PARTIALS, N.WAVE_ROW_MAX_D, N.D_BREAKS)
    assert g["max_d"] >= 8192 and g["reg_max_d"] <= g["max_d"] and g["d_breaks"][-1] == g["max_d"]
    assert g["rows_per_block"] == g["partials"] == g["ws_bytes"] == 0
    for n, d in ((1, 1), (5, 768), (4097, 768), (100000, 768), (3, 1025), (5000, 8192)):
        q = N.geometry(n, d)
        rpb = g["threads"] // 64 if d <= g["wave_row_max_d"] else 1
        assert q["rows_per_block"] == rpb and q["row_blocks"] == -(-n // rpb)
        assert q["partials"] == min(q["row_blocks"], g["max_partials"]) == N._partials(n, d)
        assert q["ws_bytes"] == q["partials"] * d * 4
    # refused before any launch: these never touch the (fake, aligned) pointers
    fwd = dict(x=4096, ld_x=8, residual=8192, ld_residual=8, h=12288, ld_h=8, y=16384, ld_y=8, w=20480, N=2, D=8,
               eps=1e-6, dtype=_lib.BF16)
    bwd = dict(h=4096, ld_h=8, dy=8192, ld_dy=8, dh=12288, ld_dh=8, w=20480, dw=24576, ws=28672, ws_bytes=N.geometry(2, 8)["ws_bytes"],
               N=2, D=8, eps=1e-6, dtype=_lib.BF16)
    bad = [("trlx_t5_rmsnorm_fwd", fwd, dict(x=None)), ("trlx_t5_rmsnorm_fwd", fwd, dict(y=None)),
           ("trlx_t5_rmsnorm_fwd", fwd, dict(w=None)), ("trlx_t5_rmsnorm_fwd", fwd, dict(h=None)),
           ("trlx_t5_rmsnorm_fwd", fwd, dict(residual=None)), ("trlx_t5_rmsnorm_fwd", fwd, dict(ld_y=7)),
           ("trlx_t5_rmsnorm_fwd", fwd, dict(D=0)), ("trlx_t5_rmsnorm_fwd", fwd, dict(D=g["max_d"] + 1, ld_x=10 ** 5, ld_residual=10 ** 5, ld_h=10 ** 5, ld_y=10 ** 5)),
           ("trlx_t5_rmsnorm_fwd", fwd, dict(N=-1)), ("trlx_t5_rmsnorm_fwd", fwd, dict(dtype=_lib.I64)),
           ("trlx_t5_rmsnorm_fwd", fwd, dict(y=12288)), ("trlx_t5_rmsnorm_fwd", fwd, dict(y=12288 + 16)),
           ("trlx_t5_rmsnorm_fwd", fwd, dict(h=4096 + 2)), ("trlx_t5_rmsnorm_fwd", fwd, dict(x=4096 + 1)),
           ("trlx_t5_rmsnorm_bwd", bwd, dict(h=None)), ("trlx_t5_rmsnorm_bwd", bwd, dict(dy=None)),
           ("trlx_t5_rmsnorm_bwd", bwd, dict(dh=None, dw=None)), ("trlx_t5_rmsnorm_bwd", bwd, dict(w=None)),
           ("trlx_t5_rmsnorm_bwd", bwd, dict(ws=None)), ("trlx_t5_rmsnorm_bwd", bwd, dict(ws_bytes=N.geometry(2, 8)["ws_bytes"] - 1)),
           ("trlx_t5_rmsnorm_bwd", bwd, dict(ld_dh=7)), ("trlx_t5_rmsnorm_bwd", bwd, dict(dh=None, dh_in=12288, ld_dh_in=8)),
           ("trlx_t5_rmsnorm_bwd", bwd, dict(dh=4096))]
    for entry, base, change in bad:
        with pytest.raises(ValueError):
            _lib.call(entry, ctypes.byref(_lib.T5RmsNormArgs(**{**base, **change})), None)
    assert _lib.call("trlx_t5_rmsnorm_fwd", ctypes.byref(_lib.T5RmsNormArgs(**{**fwd, "N": 0})), None) == 0


# ------------------------------------------------------------------ T5LayerNorm and the torch route
def test_state_dict_loads_both_ways():
    hf_t5 = pytest.importorskip("transformers.models.t5.modeling_t5")
    hf = hf_t5.T5LayerNorm(24, eps=1e-5)
    with torch.no_grad():
        hf.weight.copy_(torch.randn(24, generator=torch.Generator().manual_seed(3)))
    m = P.T5LayerNorm(24, eps=1e-5)
    assert list(m.state_dict()) == list(hf.state_dict()) == ["weight"] and m.variance_epsilon == hf.variance_epsilon
    assert torch.equal(m.weight, torch.ones(24))
    m.load_state_dict(hf.state_dict(), strict=True)
    other = hf_t5.T5LayerNorm(24)
    other.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(other.weight, hf.weight)
    h = torch.randn(2, 3, 24, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    assert float((m.double()(h) - hf.double()(h)).abs().max()) <= 2e-6   # HF's variance is fp32 even here


def test_other_dtypes_take_hf_expressions():
    c = C.case(3, 5, torch.float32, special=False)
    x, r, w = c["x"].double(), c["residual"].double(), c["w"].double()
    h, y = P.t5_add_rmsnorm(x, r, w)
    assert torch.equal(h, r + x) and torch.equal(y, C.norm64(r + x, w)) and torch.equal(P.t5_rmsnorm(r + x, w), y)
    for dt, wdt in ((torch.float16, torch.float16), (torch.bfloat16, torch.float32), (torch.float16, torch.float32)):
        hh, ww = (r + x).to(dt), w.to(wdt)                       # fp16, and HF's fp32-weight case
        assert torch.equal(P.t5_rmsnorm(hh, ww), C.hf_norm(hh, ww))
        h2, y2 = P.T5LayerNorm(5).to(wdt).add_forward(x.to(dt), r.to(dt))
        assert torch.equal(h2, r.to(dt) + x.to(dt)) and torch.equal(y2, C.hf_norm(h2, torch.ones(5, dtype=wdt)))
    wide = torch.randn(2, P.t5_norm.MAX_D + 8)                   # D over the limit: torch, on any device
    assert torch.equal(P.t5_rmsnorm(wide, torch.ones(wide.shape[-1])), C.hf_norm(wide, torch.ones(wide.shape[-1])))
    xg, rg, wg = x.clone().requires_grad_(), r.clone().requires_grad_(), w.clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b, ww: P.t5_add_rmsnorm(a, b, ww), (xg, rg, wg))
    assert torch.autograd.gradcheck(lambda a, ww: P.t5_rmsnorm(a, ww), (xg, wg))


def test_argument_errors(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", no_library)
    monkeypatch.setattr(_lib, "load", no_library)
    h, w = torch.zeros(2, 3, 8), torch.ones(8)
    with pytest.raises(ValueError, match="share shape, dtype and device"):
        P.t5_add_rmsnorm(h, h[:, :2], w)
    with pytest.raises(ValueError, match="share shape, dtype and device"):
        P.t5_add_rmsnorm(h, h.to(torch.bfloat16), w)
    with pytest.raises(ValueError, match=r"weight must be \[D\]"):
        P.t5_rmsnorm(h, torch.ones(7))
    with pytest.raises(ValueError, match=r"weight must be \[D\]"):
        P.t5_rmsnorm(h, torch.ones(1, 8))
    with pytest.raises(ValueError, match="D >= 1"):
        P.t5_rmsnorm(torch.zeros(4, 0), torch.ones(0))
    with pytest.raises(ValueError, match="D >= 1"):
        P.t5_rmsnorm(torch.zeros(()), w)
    with pytest.raises(TypeError):
        P.t5_rmsnorm([1.0, 2.0], w)
    for dt in (torch.float32, torch.bfloat16):                   # kernel dtypes off the device: as t5_ff_act
        with pytest.raises(ValueError, match="no CPU path"):
            P.t5_rmsnorm(h.to(dt), w.to(dt))
        with pytest.raises(ValueError, match="no CPU path"):
            P.T5LayerNorm(8).to(dt).add_forward(h.to(dt), h.to(dt))
