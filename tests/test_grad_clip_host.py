"""Host-side checks of the global-norm gradient clip (no GPU): the header, the binding and the
library agree on the new entries and on the layout of their structs; every refusal of
trlx_grad_norm and trlx_adamw_step_clipped, with made-up addresses and no launch; the argument
checks of the Python layer; max_grad_norm stays out of param_groups and state_dict; and the
acceptance rule of the GPU test (adamw_checks.accepted against grad_clip_checks' fp64 oracle)
rejects four deliberately wrong restatements of the clip and accepts the right one."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import adamw_checks as C
import grad_clip_checks as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trlx_t5_amd.h")
OK, ERR_SHAPE, ERR_DTYPE, ERR_ARG = 0, 1, 3, 5
BASE = 0x7000_0000_0000  # made-up device addresses: nothing is launched, nothing dereferenced
RECORD, WORKSPACE = BASE + (64 << 20), BASE + (65 << 20)
CHUNK = _lib.ADAMW_CHUNK


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "trlx-t5_amd", "csrc"), "-j8"])
    return _lib.load()


def grad(k=0, n=100, dtype=_lib.F32, **over):
    """One live gradient at BASE + k MiB (16-B aligned, disjoint from the others)."""
    e = dict(g=BASE + (k << 20), dtype=dtype, numel=n)
    e.update(over)
    return e


def norm_call(lib, entries, max_norm=1.0, record=RECORD, workspace=WORKSPACE, workspace_bytes=1 << 16, scale=1,
              with_lists=True):
    n = len(entries)
    a = _lib.GradNormArgs()
    a.count = n
    g = (ctypes.c_void_p * max(n, 1))(*[e["g"] for e in entries])
    dt = (ctypes.c_int * max(n, 1))(*[e["dtype"] for e in entries])
    numel = (ctypes.c_int64 * max(n, 1))(*[e["numel"] for e in entries])
    if with_lists:
        a.g, a.g_dtype, a.numel = g, dt, numel
    a.max_norm, a.record, a.workspace, a.workspace_bytes, a.scale_in_place = max_norm, record, workspace, \
        workspace_bytes, scale
    rc = lib.trlx_grad_norm(ctypes.byref(a), None)
    return rc, lib.trlx_last_error().decode()


def workspace_bytes(lib, numels):
    arr = (ctypes.c_int64 * max(len(numels), 1))(*numels)
    return lib.trlx_grad_norm_workspace_bytes(arr, len(numels))


# ------------------------------------------------------------------ header, binding, export, layout
NEW_ENTRIES = {
    "trlx_grad_norm_workspace_bytes": r"^int64_t trlx_grad_norm_workspace_bytes\(const int64_t\* numel, int64_t count\);",
    "trlx_grad_norm": r"^int trlx_grad_norm\(const trlx_grad_norm_args\* args, void\* stream\);",
    "trlx_adamw_step_clipped":
        r"^int trlx_adamw_step_clipped\(const trlx_adamw_args\* args, const void\* record, void\* stream\);",
}


def test_header_declares_and_binding_lists_the_new_entries():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, decl in NEW_ENTRIES.items():
        assert re.search(decl, txt, flags=re.M), name
        assert name in _lib.SIGNATURES, name
    # the existing step is declared as before and the change is additive
    assert re.search(r"^int trlx_adamw_step\(const trlx_adamw_args\* args, void\* stream\);", txt, flags=re.M)
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", txt) and _lib.ABI_VERSION == 2
    assert "clip_grad_norm_" in P.__all__ and callable(P.clip_grad_norm_)


def test_library_exports_the_new_entries(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (trlx_\w+)", out))
    assert set(NEW_ENTRIES) <= exported


@pytest.mark.parametrize("mirror, c_name", [(_lib.GradNormArgs, "trlx_grad_norm_args"),
                                            (_lib.GradNormRecord, "trlx_grad_norm_record"),
                                            (_lib.AdamwArgs, "trlx_adamw_args")])
def test_struct_mirrors_match_the_header(tmp_path, mirror, c_name):
    fields = [f[0] for f in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields)
                   + f'printf("%zu\\n", sizeof({c_name}));\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [getattr(mirror, f).offset for f in fields] + [ctypes.sizeof(mirror)]


def test_record_is_32_bytes_and_python_reads_it_as_eight_floats():
    assert ctypes.sizeof(_lib.GradNormRecord) == 32 and P.optim.RECORD_FLOATS == 8
    r = _lib.GradNormRecord
    # the views optim.py takes of a float32[8] record: norm [0], coef [1], nonfinite int32 [2], sumsq float64 [2]
    assert (r.norm.offset, r.coef.offset, r.nonfinite.offset, r.sumsq.offset) == (0, 4, 8, 16)


def test_workspace_bytes(lib):
    assert workspace_bytes(lib, [100]) == 8
    assert workspace_bytes(lib, [0]) == 8 and workspace_bytes(lib, []) == 8  # never empty: NULL is refused
    assert workspace_bytes(lib, [CHUNK]) == 8 and workspace_bytes(lib, [CHUNK + 1]) == 16
    assert workspace_bytes(lib, [3 * CHUNK + 7, 0, 5]) == 8 * 5
    assert workspace_bytes(lib, [5, -1]) == -1
    assert lib.trlx_grad_norm_workspace_bytes(None, 2) == -1


# ------------------------------------------------------------------ refusals, nothing launched
def test_refuses_null_args_and_lists(lib):
    assert lib.trlx_grad_norm(None, None) == ERR_ARG
    assert "NULL trlx_grad_norm_args" in lib.trlx_last_error().decode()
    rc, msg = norm_call(lib, [grad()], with_lists=False)
    assert rc == ERR_ARG and "tensor list" in msg


def test_refuses_null_pointer_in_a_live_entry(lib):
    rc, msg = norm_call(lib, [grad(0), grad(1, g=None)])
    assert rc == ERR_ARG and "tensor 1: NULL pointer" in msg


def test_refuses_null_record_and_null_workspace(lib):
    rc, msg = norm_call(lib, [grad()], record=None)
    assert rc == ERR_ARG and "NULL grad-norm record" in msg
    rc, msg = norm_call(lib, [grad()], workspace=None)
    assert rc == ERR_ARG and "NULL grad-norm workspace" in msg


def test_refuses_a_workspace_that_is_too_small(lib):
    entries = [grad(0, n=3 * CHUNK + 7), grad(8, n=5, dtype=_lib.BF16)]
    need = workspace_bytes(lib, [e["numel"] for e in entries])
    assert need == 8 * 5
    rc, msg = norm_call(lib, entries, workspace_bytes=need - 8)
    assert rc == ERR_ARG and f"workspace of {need - 8} bytes, {need} needed" in msg
    rc, msg = norm_call(lib, entries, workspace_bytes=0)
    assert rc == ERR_ARG and "needed" in msg


@pytest.mark.parametrize("off", [1, 2, 4])
def test_refuses_a_record_not_aligned_to_8_bytes(lib, off):
    rc, msg = norm_call(lib, [grad()], record=RECORD + off)
    assert rc == ERR_ARG and "record is not aligned to 8 bytes" in msg


@pytest.mark.parametrize("dtype", [_lib.I64, 7, -1])
def test_refuses_unsupported_dtype(lib, dtype):
    rc, msg = norm_call(lib, [grad(0), grad(1, dtype=dtype)])
    assert rc == ERR_DTYPE and f"tensor 1: dtype {dtype}" in msg


@pytest.mark.parametrize("dtype, off", [(_lib.F32, 1), (_lib.F32, 2), (_lib.BF16, 1)])
def test_refuses_gradient_not_aligned_to_its_element(lib, dtype, off):
    rc, msg = norm_call(lib, [grad(0, dtype=dtype), grad(1, dtype=dtype, g=BASE + (1 << 20) + off)])
    assert rc == ERR_ARG and "tensor 1: g not aligned to the element size" in msg


@pytest.mark.parametrize("max_norm", [float("nan"), -1.0, -0.001, float("-inf")])
def test_refuses_nan_or_negative_max_norm(lib, max_norm):
    rc, msg = norm_call(lib, [grad()], max_norm=max_norm)
    assert rc == ERR_ARG and "max_norm" in msg


@pytest.mark.parametrize("dtype, es", [(_lib.F32, 4), (_lib.BF16, 2)])
def test_refuses_record_or_workspace_overlapping_a_gradient(lib, dtype, es):
    n = 1000
    e = grad(1, n=n, dtype=dtype)
    lo, hi = e["g"], e["g"] + n * es
    for record in (lo, hi - 8, lo - 24):  # first bytes, last bytes, the record's last 8 bytes on g's first
        rc, msg = norm_call(lib, [grad(0, dtype=dtype), e], record=record)
        assert rc == ERR_ARG and "tensor 1: the record overlaps g" in msg, hex(record)
    for ws in (lo, hi - 8, lo - 64 + 8):
        rc, msg = norm_call(lib, [grad(0, dtype=dtype), e], workspace=ws, workspace_bytes=64)
        assert rc == ERR_ARG and "tensor 1: the workspace overlaps g" in msg, hex(ws)
    rc, msg = norm_call(lib, [e], record=WORKSPACE + 8)
    assert rc == ERR_ARG and "record overlaps the workspace" in msg


def test_refuses_bad_numel_and_scale_mode(lib):
    rc, msg = norm_call(lib, [grad(n=-1)])
    assert rc == ERR_SHAPE and "numel -1" in msg
    rc, msg = norm_call(lib, [grad(0), dict(g=1 << 56, dtype=_lib.F32, numel=1 << 50)], workspace_bytes=1 << 60)
    assert rc == ERR_SHAPE and "tensor 1 too large" in msg
    rc, msg = norm_call(lib, [grad()], scale=3)
    assert rc == ERR_ARG and "scale_in_place 3" in msg


def adamw_args(n=100):
    a = _lib.AdamwArgs()
    a.p_dtype, a.g_dtype, a.count = _lib.F32, _lib.F32, 1
    cols = [(ctypes.c_void_p * 1)(BASE + (k << 20)) for k in range(4)]
    a.p, a.g, a.m, a.v = cols
    a.numel = (ctypes.c_int64 * 1)(n)
    a.step, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.alpha = 1, 1e-3, 0.9, 0.95, 1e-8, 1e-2, 0.5
    return a, cols


def test_clipped_step_refusals(lib):
    a, keep = adamw_args()
    assert lib.trlx_adamw_step_clipped(None, RECORD, None) == ERR_ARG
    assert lib.trlx_adamw_step_clipped(ctypes.byref(a), None, None) == ERR_ARG
    assert "NULL grad-norm record" in lib.trlx_last_error().decode()
    assert lib.trlx_adamw_step_clipped(ctypes.byref(a), RECORD + 4, None) == ERR_ARG
    assert "not aligned to 8 bytes" in lib.trlx_last_error().decode()
    for k, name in enumerate("pgmv"):  # a record inside any tensor of the step
        assert lib.trlx_adamw_step_clipped(ctypes.byref(a), BASE + (k << 20) + 392, None) == ERR_ARG
        assert f"the clip record overlaps {name}" in lib.trlx_last_error().decode()
    # the step's own refusals still come first-hand
    a.step = 0
    assert lib.trlx_adamw_step_clipped(ctypes.byref(a), RECORD, None) == ERR_ARG
    assert "step 0" in lib.trlx_last_error().decode()
    a.step, a.g_dtype = 1, _lib.I64
    assert lib.trlx_adamw_step_clipped(ctypes.byref(a), RECORD, None) == ERR_DTYPE


# ------------------------------------------------------------------ Python layer, no device
def with_grad(*shape, dtype=torch.float32):
    p = torch.nn.Parameter(torch.zeros(*shape, dtype=dtype))
    p.grad = torch.ones(*shape, dtype=dtype)
    return p


def test_clip_grad_norm_argument_checks():
    w = [with_grad(3)]
    for nt in (1.0, float("inf"), 3, 2.5):
        with pytest.raises(ValueError, match="norm_type"):
            P.clip_grad_norm_(w, 1.0, norm_type=nt)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            P.clip_grad_norm_(w, bad)
    with pytest.raises(ValueError, match="ROCm"):  # no CPU path
        P.clip_grad_norm_(w, 1.0)
    with pytest.raises(ValueError, match="unsupported gradient dtype"):
        P.clip_grad_norm_([with_grad(3, dtype=torch.float64)], 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        p = with_grad(3, 4)
        p.grad = torch.ones(4, 3).t()
        P.clip_grad_norm_([p], 1.0)


def test_no_gradients_returns_what_torch_returns():
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    want = torch.nn.utils.clip_grad_norm_(ps, 1.0)
    for got in (P.clip_grad_norm_(ps, 1.0), P.clip_grad_norm_([], 1.0), P.clip_grad_norm_(ps[0], 1.0)):
        assert got.dtype == want.dtype and got.shape == want.shape and got.device == want.device
        assert torch.equal(got, want)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("-inf")])
def test_negative_or_nan_max_grad_norm_raises(bad):
    w = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="max_grad_norm"):
        P.FusedAdamW(w, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        P.FusedAdamW(w).step(max_grad_norm=bad)
    p, g, m, v = (torch.zeros(4) for _ in range(4))
    with pytest.raises(ValueError, match="max_grad_norm"):
        P.adamw_step([p], [g], [m], [v], step=1, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0,
                     max_grad_norm=bad)


def test_max_grad_norm_is_keyword_only_and_a_record_needs_it():
    w = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(TypeError):
        P.FusedAdamW(w, 1e-3, (0.9, 0.999), 1e-8, 1e-2, False, False, False, 1.0)
    with pytest.raises(TypeError):
        P.FusedAdamW(w).step(None, None, 1.0)
    p, g, m, v = (torch.zeros(4) for _ in range(4))
    with pytest.raises(ValueError, match="give max_grad_norm too"):
        P.adamw_step([p], [g], [m], [v], step=1, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0,
                     grad_norm_record=torch.zeros(8))


def test_max_grad_norm_stays_out_of_param_groups_and_state_dict():
    def params():
        g = torch.Generator().manual_seed(3)
        return [torch.nn.Parameter(torch.randn(3, 4, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g))]

    ours = P.FusedAdamW([{"params": params()[:1], "lr": 5e-4}, {"params": params()[1:]}], lr=2e-3, max_grad_norm=1.0)
    plain = P.FusedAdamW(params())
    assert ours.max_grad_norm == 1.0 and plain.max_grad_norm is None
    assert ours.grad_norm is None and ours.clip_coef is None  # no clipped step yet
    assert "max_grad_norm" not in ours.defaults
    for group in ours.param_groups:
        assert "max_grad_norm" not in group
    sd = ours.state_dict()
    theirs = torch.optim.AdamW([{"params": params()[:1]}, {"params": params()[1:]}], lr=1e-3)
    assert all(set(a) == set(b) for a, b in zip(sd["param_groups"], theirs.state_dict()["param_groups"]))
    assert "max_grad_norm" not in repr(sd)
    # FusedAdamW -> torch -> FusedAdamW
    theirs.load_state_dict(sd)
    assert [g["lr"] for g in theirs.param_groups] == [5e-4, 2e-3]
    for p in (q for g in theirs.param_groups for q in g["params"]):
        p.grad = torch.ones_like(p)
    theirs.step()
    back = P.FusedAdamW([{"params": params()[:1]}, {"params": params()[1:]}], max_grad_norm=0.5)
    back.load_state_dict(theirs.state_dict())
    assert back.max_grad_norm == 0.5  # not part of the state: the loaded dict does not touch it
    assert [g["lr"] for g in back.param_groups] == [5e-4, 2e-3]
    for p in (q for g in back.param_groups for q in g["params"]):
        assert float(back.state[p]["step"]) == 1.0 and set(back.state[p]) == {"step", "exp_avg", "exp_avg_sq"}


def test_a_clipped_step_without_gradients_does_nothing():
    w = [torch.nn.Parameter(torch.ones(3))]
    opt = P.FusedAdamW(w, max_grad_norm=1.0)
    assert opt.step() is None and len(opt.state) == 0 and opt.grad_norm is None
    assert opt.step(lambda: torch.tensor(2.5), max_grad_norm=0.1) == 2.5


def test_step_and_sync_takes_max_grad_norm_by_keyword_only():
    heads = P.ILQLHeads(P.ILQLConfig(), 8, 11)
    seen = {}

    class Spy:
        def step(self, closure=None, **kw):
            seen.update(kw)

    heads.step_and_sync(Spy())
    assert set(seen) == {"polyak"}  # left out: the optimizer's own value holds
    heads.step_and_sync(Spy(), max_grad_norm=1.0)
    assert seen["max_grad_norm"] == 1.0
    heads.step_and_sync(Spy(), max_grad_norm=None)
    assert seen["max_grad_norm"] is None
    with pytest.raises(TypeError):
        heads.step_and_sync(Spy(), None, 1.0)


# ------------------------------------------------------------------ the rule can see a wrong clip
SIZES, G_DTYPES, STEPS, WD = [4099, 257], [torch.float32, torch.bfloat16], 10, 1e-2


def restated(params, grads, variant):
    """The clip restated with fp32 torch ops on the CPU — the fp64 norm rounded to fp32, the
    coefficient as torch forms it, one rounding per op — then torch's fp32 AdamW; `variant`
    plants one error.  Returns run_optimizer's per-step records."""
    def clipped(gs):
        def coef_of(norm):
            c = G.MAX_NORM / norm if variant == "no_eps" else (norm + 1e-6).reciprocal() * G.MAX_NORM
            return c if variant == "unclamped" else torch.clamp(c, max=1.0)

        total = torch.tensor(G.norm64(gs), dtype=torch.float64).float()
        out = []
        for g in gs:
            coef = coef_of(torch.tensor(G.norm64([g]), dtype=torch.float64).float() if variant == "per_tensor" else total)
            s = g.float() * coef
            if g.dtype == torch.bfloat16 and variant != "bf16_not_rerounded":
                s = s.bfloat16().float()
            out.append(s)
        return out

    ps = [p.clone().requires_grad_(True) for p in params]
    return C.run_optimizer(lambda q: torch.optim.AdamW(q, lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=WD),
                           ps, [clipped(gs) for gs in grads])


@pytest.fixture(scope="module")
def sensitivity_problem():
    params, grads = G.make_clip_problem(SIZES, STEPS, seed=31, g_dtypes=G_DTYPES)
    norms = [G.norm64(gs) for gs in grads]
    # the clip is active on the odd steps and idle on the even ones
    assert all(n > 1.5 * G.MAX_NORM for n in norms[0::2]) and all(n < 0.5 * G.MAX_NORM for n in norms[1::2])
    oracle = G.oracle_run_clipped(params, grads, WD, G.MAX_NORM)

    class Holder:
        def __init__(self, g):
            self.grad = g.clone()

    def torch_clipped(gs):
        """torch's own fp32 route: its total norm over the gradients' fp32 values (its norm of a
        bf16 tensor is itself rounded to bf16, an error of 2^-9 that would hide every variant
        below), its coefficient, its in-place multiply on the stored dtypes, its fp32 AdamW."""
        hs = [Holder(g) for g in gs]
        total = torch.nn.utils.get_total_norm([g.float() for g in gs])
        torch.nn.utils.clip_grads_with_norm_(hs, G.MAX_NORM, total)
        return [h.grad.float() for h in hs]

    ps = [p.clone().requires_grad_(True) for p in params]
    torch32 = C.run_optimizer(lambda q: torch.optim.AdamW(q, lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=WD),
                              ps, [torch_clipped(gs) for gs in grads])
    return params, grads, oracle, torch32


def errors(run, oracle, step):
    r, o = run[step - 1], oracle[step - 1]
    return C.compare(r["p"], r["m"], r["v"], o)


@pytest.mark.parametrize("variant", ["no_eps", "unclamped", "per_tensor", "bf16_not_rerounded"])
def test_rule_rejects_a_wrong_clip(sensitivity_problem, variant):
    """After step 2 every variant has met a clipped step and an unclipped one."""
    params, grads, oracle, torch32 = sensitivity_problem
    wrong = restated(params, grads, variant)
    for step in (2, 10):
        e_torch, e_wrong = errors(torch32, oracle, step), errors(wrong, oracle, step)
        print(variant, step, "e_wrong", e_wrong, "e_torch", e_torch)
        # torch's fp32 route is itself close: m and v to a few fp32 roundings, p (|p| up to ~4.5, one
        # ulp there is 4.8e-7 = 4.8e-4 units of lr) to about one ulp per step over ten steps
        assert 0 < e_torch["m"] < 1e-5 and 0 < e_torch["v"] < 1e-5 and 0 < e_torch["p"] < 5e-3, e_torch
        assert not C.accepted(e_wrong, e_torch), (variant, step, e_wrong, e_torch)


def test_rule_accepts_the_right_clip(sensitivity_problem):
    params, grads, oracle, torch32 = sensitivity_problem
    right = restated(params, grads, "right")
    for step in (1, 2, 10):
        e_torch, e_right = errors(torch32, oracle, step), errors(right, oracle, step)
        print(step, "e_right", e_right, "e_torch", e_torch)
        assert C.accepted(e_right, e_torch), (step, e_right, e_torch)


def test_fp64_restatement_on_a_hand_checked_case():
    g = [torch.tensor([3.0, 0.0]), torch.tensor([4.0]).bfloat16()]
    norm, coef, out = G.clip64(g, 1.0)
    assert norm == 5.0 and coef == 1.0 / (5.0 + 1e-6)
    assert torch.equal(out[0], torch.tensor([3.0 * coef, 0.0], dtype=torch.float64))
    assert torch.equal(out[1], torch.tensor([4.0 * coef]).bfloat16().double())  # re-rounded to bf16
    assert G.clip64(g, 10.0)[1] == 1.0 and G.clip64(g, float("inf"))[1] == 1.0
    assert G.f32_ulp(1.0) == 2.0 ** -23 and G.f32_ulp(3.0) == 2.0 ** -22
