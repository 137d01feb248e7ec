"""Host-side checks of the fused AdamW (no GPU): every refusal of trlx_adamw_step on the built
library, with made-up addresses and no launch; the acceptance rule of the GPU tests
(adamw_checks.compare, e <= 2 * e_torch) rejects three deliberately wrong fp32 restatements of
the update and accepts the right one; FusedAdamW and torch.optim.AdamW exchange state_dicts
(structure only, no step); argument validation of the Python layer; the ctypes mirror of
trlx_adamw_args has the C compiler's layout."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import adamw_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trlx_t5_amd.h")
OK, ERR_SHAPE, ERR_DTYPE, ERR_ARG = 0, 1, 3, 5
BASE = 0x7000_0000_0000  # made-up device addresses: nothing is launched, nothing dereferenced


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "trlx-t5_amd", "csrc"), "-j8"])
    return _lib.load()


def entry(n=100, stride=1 << 20, **over):
    """One live table entry: p, g, m, v, master, target at BASE + k·stride (16-B aligned, disjoint)."""
    e = dict(p=BASE, g=BASE + stride, m=BASE + 2 * stride, v=BASE + 3 * stride, master=None, target=None, numel=n)
    e.update(over)
    return e


def adamw_call(lib, entries, p_dtype=_lib.F32, g_dtype=_lib.F32, step=1, lr=1e-3, alpha=0.5, with_lists=True):
    n = len(entries)
    a = _lib.AdamwArgs()
    a.p_dtype, a.g_dtype, a.count = p_dtype, g_dtype, n
    keep = []
    for k in ("p", "g", "m", "v", "master", "target"):
        col = (ctypes.c_void_p * max(n, 1))(*[e[k] for e in entries])
        keep.append(col)
        if with_lists:
            setattr(a, k, col)
    numel = (ctypes.c_int64 * max(n, 1))(*[e["numel"] for e in entries])
    if with_lists:
        a.numel = numel
    a.step, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.alpha = step, lr, 0.9, 0.95, 1e-8, 1e-2, alpha
    rc = lib.trlx_adamw_step(ctypes.byref(a), None)
    return rc, lib.trlx_last_error().decode()


def test_header_binding_and_export():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"^int trlx_adamw_step\(const trlx_adamw_args\* args, void\* stream\);", txt, flags=re.M)
    assert "trlx_adamw_step" in _lib.SIGNATURES
    for name, val in (("TRLX_ADAMW_MAX_TENSORS", _lib.ADAMW_MAX_TENSORS), ("TRLX_ADAMW_CHUNK", _lib.ADAMW_CHUNK)):
        m = re.search(rf"#define {name} (\d+)", txt)
        assert m and int(m.group(1)) == val
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", txt) and _lib.ABI_VERSION == 2  # additive change
    assert "FusedAdamW" in P.__all__ and "adamw_step" in P.__all__


def test_library_exports_the_entry(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "trlx_adamw_step" in set(re.findall(r"\bT (trlx_\w+)", out))
    assert lib.trlx_abi_version() == 2


def test_args_layout_matches_header(tmp_path):
    fields = [f[0] for f in _lib.AdamwArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(trlx_adamw_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(trlx_adamw_args));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [getattr(_lib.AdamwArgs, f).offset for f in fields] + [ctypes.sizeof(_lib.AdamwArgs)]


# ------------------------------------------------------------------ refusals, nothing launched
def test_nothing_to_do_is_ok_without_a_device(lib):
    assert adamw_call(lib, [])[0] == OK
    # zero-length tensors are skipped whatever their pointers are
    assert adamw_call(lib, [entry(n=0, p=None, g=3, m=None, v=1)])[0] == OK


def test_refuses_null_args_and_lists(lib):
    assert lib.trlx_adamw_step(None, None) == ERR_ARG
    assert "NULL trlx_adamw_args" in lib.trlx_last_error().decode()
    rc, msg = adamw_call(lib, [entry()], with_lists=False)
    assert rc == ERR_ARG and "tensor list" in msg


@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
def test_refuses_null_pointer_in_a_live_entry(lib, which):
    rc, msg = adamw_call(lib, [entry(), entry(**{which: None})])
    assert rc == ERR_ARG and "tensor 1: NULL pointer" in msg


@pytest.mark.parametrize("p_dtype, g_dtype, word", [(_lib.I64, _lib.F32, "parameter dtype 2"),
                                                    (_lib.F32, _lib.I64, "gradient dtype 2"),
                                                    (7, _lib.BF16, "parameter dtype 7"),
                                                    (_lib.BF16, -1, "gradient dtype -1")])
def test_refuses_unsupported_dtype(lib, p_dtype, g_dtype, word):
    rc, msg = adamw_call(lib, [entry()], p_dtype=p_dtype, g_dtype=g_dtype)
    assert rc == ERR_DTYPE and word in msg


@pytest.mark.parametrize("p_dtype, g_dtype, which, off", [
    (_lib.F32, _lib.F32, "p", 2), (_lib.F32, _lib.F32, "g", 1), (_lib.F32, _lib.BF16, "g", 1),
    (_lib.BF16, _lib.F32, "p", 1), (_lib.BF16, _lib.BF16, "m", 2), (_lib.BF16, _lib.BF16, "v", 3),
    (_lib.BF16, _lib.F32, "master", 2), (_lib.F32, _lib.F32, "target", 2), (_lib.BF16, _lib.F32, "target", 1)])
def test_refuses_pointer_not_aligned_to_its_element(lib, p_dtype, g_dtype, which, off):
    e = entry(master=BASE + (4 << 20) if p_dtype == _lib.BF16 else None, target=BASE + (5 << 20))
    e[which] += off
    rc, msg = adamw_call(lib, [e], p_dtype=p_dtype, g_dtype=g_dtype)
    assert rc == ERR_ARG and f"{which} not aligned to the element size" in msg


NAMES = ["p", "g", "m", "v", "master", "target"]


@pytest.mark.parametrize("x, y", [(x, y) for i, x in enumerate(NAMES) for y in NAMES[i + 1:]])
def test_refuses_any_aliasing_within_an_entry(lib, x, y):
    n = 1000
    e = entry(n=n, master=BASE + (4 << 20), target=BASE + (5 << 20))
    for off in (1996, -1996):  # the last / first four bytes of the shorter range (2000 bytes) overlap
        e[y] = e[x] + off
        rc, msg = adamw_call(lib, [entry(n=n), e], p_dtype=_lib.BF16, g_dtype=_lib.BF16)
        assert rc == ERR_ARG and f"tensor 1: {x} and {y} alias" in msg
    e[y] = e[x]  # the same tensor twice
    rc, msg = adamw_call(lib, [e], p_dtype=_lib.BF16, g_dtype=_lib.BF16)
    assert rc == ERR_ARG and f"{x} and {y} alias" in msg


def test_refuses_master_for_fp32_parameter(lib):
    rc, msg = adamw_call(lib, [entry(master=BASE + (4 << 20))])
    assert rc == ERR_ARG and "master is for a bf16 parameter" in msg


def test_refuses_tensor_too_large_for_the_grid(lib):
    big = 1 << 50
    e = dict(p=1 << 56, g=2 << 56, m=3 << 56, v=4 << 56, master=None, target=None, numel=big)
    rc, msg = adamw_call(lib, [entry(), e])
    assert rc == ERR_SHAPE and "tensor 1 too large" in msg
    rc, msg = adamw_call(lib, [entry(n=-1)])
    assert rc == ERR_SHAPE and "numel -1" in msg


def test_refuses_bad_scalars(lib):
    rc, msg = adamw_call(lib, [entry()], step=0)
    assert rc == ERR_ARG and "step 0" in msg
    rc, msg = adamw_call(lib, [entry()], lr=float("nan"))
    assert rc == ERR_ARG and "NaN" in msg
    rc, msg = adamw_call(lib, [entry(target=BASE + (5 << 20))], alpha=float("nan"))
    assert rc == ERR_ARG and "alpha is NaN" in msg


# ------------------------------------------------------------------ the rule can see a wrong optimizer
def restated(params, grads, weight_decay, variant):
    """AdamW restated with fp32 torch ops on the CPU, one op per rounding; `variant` plants one
    error.  Returns the per-step records run_optimizer returns."""
    b1, b2 = C.BETAS
    ps = [p.clone() for p in params]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    out = []
    for step, (lr, gs) in enumerate(zip(C.cosine_lrs(len(grads)), grads), start=1):
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        if variant == "no_bias_correction":
            bc1 = bc2 = 1.0
        for p, g, m, v in zip(ps, gs, ms, vs):
            if variant == "coupled_decay":
                g = g + weight_decay * p
            else:
                p.mul_(1 - lr * weight_decay)
            m.add_((1 - b1) * (g - m))
            v.mul_(b2).add_((1 - b2) * (g * g))
            if variant == "eps_in_sqrt":
                denom = (v + C.EPS).sqrt() / bc2 ** 0.5
            else:
                denom = v.sqrt() / bc2 ** 0.5 + C.EPS
            p.add_(-(lr / bc1) * (m / denom))
        out.append({"p": torch.cat(ps).double(), "m": torch.cat(ms).double(), "v": torch.cat(vs).double()})
    return out


@pytest.fixture(scope="module")
def sensitivity_problem():
    wd = 1e-2
    params, grads = C.make_problem([4099, 257], 10, seed=11)
    oracle = C.oracle_run(params, grads, wd)
    ps = [p.clone().requires_grad_(True) for p in params]
    torch32 = C.run_optimizer(lambda q: torch.optim.AdamW(q, lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=wd),
                              ps, grads)
    return wd, params, grads, oracle, torch32


@pytest.mark.parametrize("variant", ["eps_in_sqrt", "no_bias_correction", "coupled_decay"])
def test_rule_rejects_a_wrong_optimizer(sensitivity_problem, variant):
    wd, params, grads, oracle, torch32 = sensitivity_problem
    wrong = restated(params, grads, wd, variant)
    for step in (1, 10):
        o = oracle[step - 1]
        e_torch = C.compare(torch32[step - 1]["p"], torch32[step - 1]["m"], torch32[step - 1]["v"], o)
        e_wrong = C.compare(wrong[step - 1]["p"], wrong[step - 1]["m"], wrong[step - 1]["v"], o)
        print(variant, step, "e_wrong", e_wrong, "e_torch", e_torch)
        assert all(0 < e_torch[k] < 1e-3 for k in "pmv"), e_torch  # torch's fp32 route is itself close
        assert not C.accepted(e_wrong, e_torch), (variant, step, e_wrong, e_torch)


def test_rule_accepts_the_right_restatement(sensitivity_problem):
    wd, params, grads, oracle, torch32 = sensitivity_problem
    right = restated(params, grads, wd, "right")
    for step in (1, 10):
        o = oracle[step - 1]
        e_torch = C.compare(torch32[step - 1]["p"], torch32[step - 1]["m"], torch32[step - 1]["v"], o)
        e_right = C.compare(right[step - 1]["p"], right[step - 1]["m"], right[step - 1]["v"], o)
        print(step, "e_right", e_right, "e_torch", e_torch)
        assert C.accepted(e_right, e_torch), (step, e_right, e_torch)


def test_compare_flags_non_finite_values(sensitivity_problem):
    _, _, _, oracle, torch32 = sensitivity_problem
    rec = {k: v.clone() for k, v in torch32[0].items()}
    rec["m"][5] = float("nan")
    rec["v"][7] = float("inf")
    e = C.compare(rec["p"], rec["m"], rec["v"], oracle[0])
    assert e["m"] == float("inf") and e["v"] == float("inf") and e["p"] < 1e-3


# ------------------------------------------------------------------ Python layer, no device
def test_state_dict_round_trip_with_torch_adamw():
    def params():
        g = torch.Generator().manual_seed(3)
        return [torch.nn.Parameter(torch.randn(3, 4, generator=g)),
                torch.nn.Parameter(torch.randn(5, generator=g).bfloat16())]

    ours = P.FusedAdamW(params(), lr=2e-3, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.1, master_weights=True)
    theirs = torch.optim.AdamW(params(), lr=1e-3)
    assert set(ours.state_dict()["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])
    # torch -> FusedAdamW: torch's keys, exp_avg / exp_avg_sq fp32 whatever the parameter's dtype
    for p in theirs.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    theirs.step()
    sd = theirs.state_dict()
    ours.load_state_dict(sd)
    assert ours.param_groups[0]["lr"] == 1e-3 and ours.param_groups[0]["betas"] == (0.9, 0.999)
    for i, p in enumerate(ours.param_groups[0]["params"]):
        st = ours.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(st["step"]) == 1.0 and st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"].float())
    # FusedAdamW -> torch: the same keys come back (an fp32 master is an extra key, bf16 only)
    ours.state[ours.param_groups[0]["params"][1]]["master"] = torch.full((5,), 1.0000001)
    back = ours.state_dict()
    assert set(back["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert set(back["state"][1]) == {"step", "exp_avg", "exp_avg_sq", "master"}
    fresh = torch.optim.AdamW(params(), lr=5e-2)
    fresh.load_state_dict(back)
    assert fresh.param_groups[0]["lr"] == 1e-3
    for i, p in enumerate(fresh.param_groups[0]["params"]):
        assert float(fresh.state[p]["step"]) == 1.0
        assert torch.equal(fresh.state[p]["exp_avg"].float(), sd["state"][i]["exp_avg"].float())
    # and a master survives FusedAdamW -> FusedAdamW in fp32 (Optimizer.load_state_dict alone would cast it)
    again = P.FusedAdamW(params(), master_weights=True)
    again.load_state_dict(back)
    m = again.state[again.param_groups[0]["params"][1]]["master"]
    assert m.dtype == torch.float32 and torch.equal(m, torch.full((5,), 1.0000001))


def test_unsupported_options_raise_value_error():
    w = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="amsgrad"):
        P.FusedAdamW(w, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        P.FusedAdamW(w, maximize=True)
    with pytest.raises(ValueError, match="complex"):
        P.FusedAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.complex64))])
    with pytest.raises(ValueError, match="learning rate"):
        P.FusedAdamW(w, lr=-1.0)
    with pytest.raises(ValueError, match="beta parameter at index 1"):
        P.FusedAdamW(w, betas=(0.9, 1.0))
    opt = P.FusedAdamW(w)
    sd = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        opt.load_state_dict(sd)
    w[0].grad = torch.zeros(3)
    with pytest.raises(ValueError, match="ROCm"):  # no CPU path
        P.FusedAdamW(w).step()
    w[0].grad = torch.sparse_coo_tensor([[0]], [1.0], (3,))
    with pytest.raises(ValueError, match="sparse"):
        P.FusedAdamW(w).step()


def test_a_parameter_without_gradient_is_skipped():
    w = [torch.nn.Parameter(torch.ones(3))]
    opt = P.FusedAdamW(w)
    assert opt.step() is None and len(opt.state) == 0
    assert opt.step(lambda: torch.tensor(2.5)) == 2.5


def test_adamw_step_argument_validation():
    p, g, m, v = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3)
    kw = dict(step=1, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0)
    with pytest.raises(ValueError, match="1 params but 2 grads"):
        P.adamw_step([p], [g, g], [m], [v], **kw)
    with pytest.raises(ValueError, match="unsupported parameter dtype"):
        P.adamw_step([p.double()], [g], [m], [v], **kw)
    with pytest.raises(ValueError, match="unsupported gradient dtype"):
        P.adamw_step([p], [g.half()], [m], [v], **kw)
    with pytest.raises(ValueError, match="exp_avg must be float32"):
        P.adamw_step([p.bfloat16()], [g], [m.bfloat16()], [v], **kw)
    with pytest.raises(ValueError, match="shape"):
        P.adamw_step([p], [g], [torch.zeros(3, 4)], [v], **kw)
    with pytest.raises(ValueError, match="contiguous"):
        P.adamw_step([p.t()], [g.t()], [m.t()], [v.t()], **kw)
    with pytest.raises(ValueError, match="master is for a bfloat16"):
        P.adamw_step([p], [g], [m], [v], masters=[torch.zeros(4, 3)], **kw)
    with pytest.raises(ValueError, match="step must be"):
        P.adamw_step([p], [g], [m], [v], **dict(kw, step=0))
    with pytest.raises(ValueError, match="ROCm"):
        P.adamw_step([p], [g], [m], [v], **kw)
    with pytest.raises(ValueError, match="targets but"):
        P.adamw_step([p], [g], [m], [v], polyak=([p, p], [p], 0.5), **kw)
