"""AdamW with a bf16 state on the GPU (trlx_adamw_step_ex with TRLX_BF16, adamw_step with bf16
moments, FusedAdamW(state_dtype="param")).

The kernel is pinned bit for bit to adamw_bf16_checks.bf16_chain_step, the CPU restatement that
test_adamw_bf16_state_cpu.py pins to torch's bf16 AdamW; every launch form is pinned to the
plain one; torch's own bf16 AdamW on the device is measured against it (one update from a shared
state: within one bf16 ulp, differing in at most 1e-3 of the elements per quantity — the CPU
figure of 6.5e-5 for exp_avg with 15x headroom) and over ten updates by the project's rule
accepted(e_fused, e_torch) against the float64 oracle.
TRLX_ADAMW_BF16_PARITY_OUT=<file>: the measured figures are written there
(profiles/adamw_bf16_state_parity.json is such a run).

Sizes: 1, 7, 8, 9 (below / at / above one 16-byte group of 8), 255, one below / at / above one
workgroup's chunk, more than two chunks; a list one longer than the launch table.
"""
import copy
import json
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import adamw_bf16_checks as B
import adamw_checks as C
import adamw_device_checks as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
CHUNK = _lib.ADAMW_CHUNK
SIZES = [1, 7, 8, 9, 255, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
LR, WD = 1e-3, 1e-2
SENTINEL = 12288.0  # 3·2^12: exact in bf16
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    yield
    path = os.environ.get("TRLX_ADAMW_BF16_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump(_FIGURES, f, indent=1, sort_keys=True)


def values(n, seed, first_step=False):
    """bf16 CPU (p, g, m, v) of n elements: gradients N(0,1)·10^U{-4..2}; a later step's m and v
    of matching scale, or zeros for the first update.  Element 0 has g = 0 wherever n > 1."""
    params, grads = C.make_problem([n], 2, seed=seed, p_dtype=BF16, g_dtype=BF16)
    p, g = params[0], grads[0][0].clone()
    if n > 1:
        g[0] = 0.0
    if first_step:
        return p, g, torch.zeros(n, dtype=BF16), torch.zeros(n, dtype=BF16)
    g0 = grads[1][0].float()
    return p, g, (0.3 * g0).to(BF16), (0.2 * g0 * g0).to(BF16)


def to_dev(*ts):
    return [t.to(DEV).clone() for t in ts]


def check_against_chain(got, start, step, lr, betas=C.BETAS, wd=WD, what=""):
    """got: (p, m, v) device tensors after the update; start: the CPU (p, g, m, v) it began from."""
    want = B.bf16_chain_step(*start, step, lr, betas, C.EPS, wd)
    for name, a, b in zip("pmv", got, want):
        B.assert_same_bits(a, b, f"{what} {name}")
    return want


# ------------------------------------------------------------------ the chain, every size
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("with_target", [False, True])
def test_every_size_is_the_chain_bit_for_bit(step, with_target):
    """All sizes in one call: step 1 from m = v = 0 (g = 0 leaves denom = bf(eps)) and a later step."""
    starts = [values(n, 40 + i, first_step=(step == 1)) for i, n in enumerate(SIZES)]
    dev = [to_dev(*s) for s in starts]
    targets0 = [torch.randn(n, generator=torch.Generator().manual_seed(90 + i)).to(BF16) for i, n in enumerate(SIZES)]
    targets = [t.to(DEV) for t in targets0]
    ps, gs, ms, vs = ([d[k] for d in dev] for k in range(4))
    alpha = 0.25
    P.adamw_step(ps, gs, ms, vs, step=step, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD,
                 polyak=(targets, ps, alpha) if with_target else None)
    for i, n in enumerate(SIZES):
        want = check_against_chain((ps[i], ms[i], vs[i]), starts[i], step, LR, what=f"n={n} step={step}")
        assert torch.equal(gs[i].cpu(), starts[i][1])  # the gradient is only read
        if with_target:
            B.assert_same_bits(targets[i], B.bf16_polyak(targets0[i], want[0], alpha), f"n={n} target")
        else:
            assert torch.equal(targets[i].cpu(), targets0[i])
        if step == 1 and n > 1:  # g = 0 from a zero state: m = v = 0 and p only decays
            assert float(ms[i][0]) == 0.0 and float(vs[i][0]) == 0.0
            assert float(ps[i][0]) == float(B.bf(starts[i][0][:1].float() * torch.tensor(1.0 - LR * WD)))


# ------------------------------------------------------------------ phases
def phased(t, offset, pad=24):
    """A copy of `t` as a view at element `offset` of a larger sentinel-filled buffer."""
    buf = torch.full((t.numel() + pad,), SENTINEL, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()]
    view.copy_(t)
    return buf, view


def check_guard(buf, offset, n):
    assert bool((buf[:offset].float() == SENTINEL).all()) and bool((buf[offset + n:].float() == SENTINEL).all())


@pytest.mark.parametrize("n", [5, CHUNK + 1])
def test_phases_share_the_bits(n):
    """Views whose four pointers share a 16-byte phase of 0, 1 and 7 elements (vector path with
    a head and a tail) and views of different phases (element path): the same bits, and nothing
    outside the views is written.  Base pointers of fresh allocations are 16-byte aligned."""
    start = values(n, 50)
    t0 = torch.randn(n, generator=torch.Generator().manual_seed(51)).to(BF16)
    want = B.bf16_chain_step(*start, 3, LR, C.BETAS, C.EPS, WD)
    for offs in ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (7, 7, 7, 7, 7), (0, 1, 3, 2, 5), (7, 7, 7, 6, 7)):
        made = [phased(t, o) for t, o in zip((*start, t0), offs)]
        for (buf, view), o in zip(made, offs):
            assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + 2 * o
        (p, g, m, v, t) = (view for _, view in made)
        P.adamw_step([p], [g], [m], [v], step=3, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD,
                     polyak=([t], [p], 0.5))
        for name, a, b in zip("pmv", (p, m, v), want):
            B.assert_same_bits(a, b, f"n={n} offsets={offs} {name}")
        B.assert_same_bits(t, B.bf16_polyak(t0, want[0], 0.5), f"n={n} offsets={offs} target")
        for (buf, _), o in zip(made, offs):
            check_guard(buf, o, n)


def test_list_one_longer_than_the_table_with_an_empty_tensor():
    sizes = [5 + (i % 3) for i in range(_lib.ADAMW_MAX_TENSORS + 1)]
    sizes[4] = 0
    starts = [values(n, 60 + i) if n else tuple(torch.zeros(0, dtype=BF16) for _ in range(4))
              for i, n in enumerate(sizes)]
    dev = [to_dev(*s) for s in starts]
    ps, gs, ms, vs = ([d[k] for d in dev] for k in range(4))
    P.adamw_step(ps, gs, ms, vs, step=2, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD)
    for i, n in enumerate(sizes):
        if n:
            check_against_chain((ps[i], ms[i], vs[i]), starts[i], 2, LR, what=f"tensor {i}")


# ------------------------------------------------------------------ special values
def test_nonfinite_gradients_follow_the_chain():
    n = 16
    p, g, m, v = values(n, 70)
    g[1], g[2], g[3] = float("inf"), float("-inf"), float("nan")
    g[9], g[10] = float("inf"), float("nan")  # the same in the second group of 8
    dp, dg, dm, dv = to_dev(p, g, m, v)
    P.adamw_step([dp], [dg], [dm], [dv], step=4, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD)
    want = check_against_chain((dp, dm, dv), (p, g, m, v), 4, LR, what="non-finite row")
    assert bool(torch.isnan(want[0][[1, 2, 3, 9, 10]].float()).all())  # inf/inf and NaN reach p
    assert bool(torch.isfinite(dp.float()[[0, 4, 5, 6, 7, 8, 11]]).all())


def test_large_v_stands_still_as_torchs_does():
    """beta2 = 0.999: bf(v·b2) == v for every bf16 v (1e-3 is below half an ulp, 2^-9 at least),
    and (1 - b2)·g² of a small g is below half an ulp too: v does not move — torch's bf16
    AdamW has the same stagnation; the chain and the kernel reproduce it."""
    n = 64
    p, _, m, _ = values(n, 71)
    v = torch.linspace(1.0, 300.0, n).to(BF16)
    g = torch.full((n,), 2.0 ** -6, dtype=BF16)
    dp, dg, dm, dv = to_dev(p, g, m, v)
    P.adamw_step([dp], [dg], [dm], [dv], step=9, lr=LR, betas=(0.9, 0.999), eps=C.EPS, weight_decay=WD)
    check_against_chain((dp, dm, dv), (p, g, m, v), 9, LR, betas=(0.9, 0.999), what="large v")
    assert torch.equal(dv.cpu(), v)


# ------------------------------------------------------------------ the launch forms
def leaves(ps):
    return [p.to(DEV).clone().requires_grad_(True) for p in ps]


def set_grads(params, gs):
    for p, g in zip(params, gs):
        p.grad = g.to(DEV).clone()


def snapshot(opt, params):
    return ([p.detach().clone() for p in params], [opt.state[p]["exp_avg"].clone() for p in params],
            [opt.state[p]["exp_avg_sq"].clone() for p in params])


def assert_snapshots_equal(a, b, what):
    for name, xs, ys in zip("pmv", a, b):
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert x.dtype == y.dtype == BF16, (what, name, i, x.dtype, y.dtype)
            B.assert_same_bits(x, y, f"{what} {name}[{i}]")


def fused(params, **kw):
    return P.FusedAdamW(params, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD, state_dtype="param", **kw)


FORM_SIZES = [7, CHUNK + 1, 33]


def form_problem(seed, steps):
    return C.make_problem(FORM_SIZES, steps, seed=seed, p_dtype=BF16, g_dtype=BF16)


def test_clipped_is_clip_then_step():
    ps, gs = form_problem(80, 2)
    a, b = leaves(ps), leaves(ps)
    oa, ob = fused(a, max_grad_norm=1.0), fused(b)
    for g in gs:
        set_grads(a, g)
        set_grads(b, g)
        oa.step()
        assert all(torch.equal(p.grad.cpu(), x) for p, x in zip(a, g))  # .grad stays unclipped
        P.clip_grad_norm_(b, 1.0)
        ob.step()
    assert float(oa.clip_coef) < 1.0
    assert_snapshots_equal(snapshot(oa, a), snapshot(ob, b), "clipped")
    # and the chain on the clipped gradient of the last update, from the state before it
    c = leaves(ps)
    oc = fused(c, max_grad_norm=1.0)
    set_grads(c, gs[0])
    oc.step()
    before = [(p.detach().cpu(), None, oc.state[p]["exp_avg"].cpu(), oc.state[p]["exp_avg_sq"].cpu()) for p in c]
    set_grads(c, gs[1])
    oc.step()
    coef = float(oc.clip_coef)
    for i, p in enumerate(c):
        start = (before[i][0], B.bf16_clip(gs[1][i], coef), before[i][2], before[i][3])
        check_against_chain((p.detach(), oc.state[p]["exp_avg"], oc.state[p]["exp_avg_sq"]), start, 2, LR,
                            what=f"clipped chain [{i}]")


def test_capturable_eager_and_replay_are_the_default_mode():
    """Three updates: the default mode with the rate set by hand, capturable eager, and one
    captured update replayed; rates and betas are a tuple on which the device's product chain
    forms the scalars of the default mode's pow (adamw_device_checks.GPU_TUPLES)."""
    betas, rates, wd, _, _ = D.GPU_TUPLES["cosine12"]
    assert betas == C.BETAS and wd == WD
    rates = rates[:3]
    ps, gs = form_problem(81, 3)
    ref = leaves(ps)
    oref = fused(ref)
    for lr, g in zip(rates, gs):
        oref.param_groups[0]["lr"] = lr
        set_grads(ref, g)
        oref.step()
    want = snapshot(oref, ref)

    eager = leaves(ps)
    oe = fused(eager, capturable=True, lr_schedule=rates, max_grad_norm=None)
    for g in gs:
        set_grads(eager, g)
        oe.step()
    assert int(oe.applied_steps) == 3
    assert_snapshots_equal(snapshot(oe, eager), want, "capturable eager")

    params = leaves(ps)
    opt = fused(params, capturable=True, lr_schedule=rates)
    static = [torch.zeros(n, dtype=BF16, device=DEV) for n in FORM_SIZES]
    for p, buf, g in zip(params, static, gs[0]):
        buf.copy_(g)
        p.grad = buf
    opt.step()  # warm-up: every buffer exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, a linear chain of launches
        opt.step()
    assert int(opt.applied_steps) == 1  # a capture runs nothing
    for g in gs[1:]:
        for buf, new in zip(static, g):
            buf.copy_(new)
        graph.replay()
    torch.cuda.synchronize()
    assert int(opt.applied_steps) == 3
    assert_snapshots_equal(snapshot(opt, params), want, "graph replay")


def test_step_with_polyak_is_step_then_polyak_update():
    ps, gs = form_problem(82, 2)
    t0 = [torch.randn(n, generator=torch.Generator().manual_seed(83 + i)).to(BF16) for i, n in enumerate(FORM_SIZES)]
    a, b = leaves(ps), leaves(ps)
    ta, tb = [t.to(DEV).clone() for t in t0], [t.to(DEV).clone() for t in t0]
    oa, ob = fused(a), fused(b)
    for g in gs:
        set_grads(a, g)
        set_grads(b, g)
        oa.step(polyak=(ta, a, 0.25))
        ob.step()
        P.polyak_update(tb, b, 0.25)
    assert_snapshots_equal(snapshot(oa, a), snapshot(ob, b), "polyak")
    for i, (x, y) in enumerate(zip(ta, tb)):
        B.assert_same_bits(x, y, f"target {i}")
        assert not torch.equal(x.cpu(), t0[i])


def test_ilql_heads_step_and_sync_with_param_state():
    torch.manual_seed(0)
    proto = P.ILQLHeads(P.ILQLConfig(), 16, 37).to(BF16)
    g = torch.Generator().manual_seed(16)
    grads = {n: torch.randn(p.shape, generator=g).to(BF16) for n, p in proto.named_parameters() if p.requires_grad}
    out = []
    for folded in (True, False):
        heads = copy.deepcopy(proto).to(DEV)
        opt = P.FusedAdamW([p for p in heads.parameters() if p.requires_grad], lr=1e-2, betas=C.BETAS,
                           state_dtype="param")
        for _ in range(2):
            for n, p in heads.named_parameters():
                if p.requires_grad:
                    p.grad = grads[n].to(DEV)
            if folded:
                heads.step_and_sync(opt)
            else:
                opt.step()
                heads.sync_target_q_heads()
        assert all(st["exp_avg"].dtype == BF16 for st in opt.state.values())
        out.append({k: v.clone() for k, v in heads.state_dict().items()})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


# ------------------------------------------------------------------ torch on the device
def test_one_update_against_torchs_bf16_adamw_on_the_device():
    """One update (number 6) from a shared state.  Each of p, m, v within one bf16 ulp of torch's
    (adamw_bf16_checks.ulp_report: the ulp at the larger of the result and the value the op
    began from), differing in at most 1e-3 of the elements."""
    n, step = 20000, 6
    p0, g, m0, v0 = values(n, 84)
    q = p0.to(DEV).clone().requires_grad_(True)
    topt = torch.optim.AdamW([q], lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD, foreach=False)
    topt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.to(DEV).clone(),
                     "exp_avg_sq": v0.to(DEV).clone()}
    q.grad = g.to(DEV)
    topt.step()
    assert topt.state[q]["exp_avg"].dtype == BF16
    dp, dg, dm, dv = to_dev(p0, g, m0, v0)
    P.adamw_step([dp], [dg], [dm], [dv], step=step, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD)
    figures = {}
    for name, got, want, start in (("p", dp, q.detach(), p0), ("m", dm, topt.state[q]["exp_avg"], m0),
                                   ("v", dv, topt.state[q]["exp_avg_sq"], v0)):
        share, worst = B.ulp_report(got, want, start=start)
        figures[name] = {"share_differing": share, "worst_ulps": worst}
    print("one update against torch's bf16 AdamW on the device:", figures)
    _FIGURES["one_update_vs_device_torch"] = dict(figures, elements=n, cap_share=1e-3, cap_ulps=1.0)
    for name, f in figures.items():
        assert f["worst_ulps"] <= 1.0, (name, f)
        assert f["share_differing"] <= 1e-3, (name, f)


def test_trajectory_by_the_projects_rule():
    """Ten updates under CosineAnnealingLR against the float64 oracle: accepted(e_fused, e_torch),
    e_torch torch's bf16 AdamW on the device measured the same way."""
    sizes = [7, CHUNK + 1, 2 * CHUNK + 5]
    params, grads = C.make_problem(sizes, 10, seed=85, p_dtype=BF16, g_dtype=BF16)
    oracle = C.oracle_run(params, grads, WD)
    t_run = C.run_optimizer(lambda ps: torch.optim.AdamW(ps, lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=WD,
                                                         foreach=False), leaves(params), grads)
    f_run = C.run_optimizer(lambda ps: P.FusedAdamW(ps, lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=WD,
                                                    state_dtype="param"), leaves(params), grads)
    steps = []
    for k in range(10):
        e_fused = C.compare(f_run[k]["p"], f_run[k]["m"], f_run[k]["v"], oracle[k])
        e_torch = C.compare(t_run[k]["p"], t_run[k]["m"], t_run[k]["v"], oracle[k])
        print("step", k + 1, "e_fused", e_fused, "e_torch", e_torch)
        steps.append({"step": k + 1, "e_fused": e_fused, "e_torch": e_torch})
    _FIGURES["trajectory_10_steps"] = {"rule": "e_fused <= 2 * e_torch for each of p, m, v", "steps": steps}
    for s in steps:
        assert C.accepted(s["e_fused"], s["e_torch"]), s


# ------------------------------------------------------------------ state dicts
def test_state_dict_round_trip_with_torch_both_ways():
    ps, gs = form_problem(86, 4)

    def torch_opt(params):
        return torch.optim.AdamW(params, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD, foreach=False)

    # ours -> torch: torch's next step starts from identical bits, so two torch runs agree
    a = leaves(ps)
    oa = fused(a)
    for g in gs[:2]:
        set_grads(a, g)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    assert all(st["exp_avg"].dtype == BF16 and st["exp_avg_sq"].dtype == BF16 for st in sd["state"].values())
    b = [p.detach().clone().requires_grad_(True) for p in a]
    ob = torch_opt(b)
    ob.load_state_dict(copy.deepcopy(sd))
    ob.param_groups[0]["foreach"] = False  # the loaded group says None: both torch runs take one implementation
    for p, q in zip(a, b):  # loaded with nothing converted
        assert torch.equal(ob.state[q]["exp_avg"], oa.state[p]["exp_avg"])
        assert torch.equal(ob.state[q]["exp_avg_sq"], oa.state[p]["exp_avg_sq"])
        assert float(ob.state[q]["step"]) == 2.0
    c = [p.detach().clone().requires_grad_(True) for p in a]
    oc = torch_opt(c)
    for p, q in zip(a, c):  # the same state set by hand
        oc.state[q] = {"step": torch.tensor(2.0), "exp_avg": oa.state[p]["exp_avg"].clone(),
                       "exp_avg_sq": oa.state[p]["exp_avg_sq"].clone()}
    set_grads(b, gs[2])
    set_grads(c, gs[2])
    ob.step()
    oc.step()
    assert_snapshots_equal(snapshot(ob, b), snapshot(oc, c), "torch after our state_dict")

    # torch -> ours: our next step from torch's checkpoint is our next step from the same bits
    d = [p.detach().clone().requires_grad_(True) for p in b]
    od = fused(d)
    od.load_state_dict(copy.deepcopy(ob.state_dict()))
    for q, r in zip(b, d):
        assert od.state[r]["exp_avg"].dtype == BF16 and torch.equal(od.state[r]["exp_avg"], ob.state[q]["exp_avg"])
        assert torch.equal(od.state[r]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])
    set_grads(d, gs[3])
    od.step()
    for i, (q, r) in enumerate(zip(b, d)):
        start = (q.detach().cpu(), gs[3][i], ob.state[q]["exp_avg"].cpu(), ob.state[q]["exp_avg_sq"].cpu())
        check_against_chain((r.detach(), od.state[r]["exp_avg"], od.state[r]["exp_avg_sq"]), start, 4, LR,
                            what=f"after torch's state_dict [{i}]")


def test_loading_an_fp32_state_checkpoint_rounds_once():
    ps, gs = form_problem(87, 2)
    a = leaves(ps)
    oa = P.FusedAdamW(a, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD)  # fp32 state
    set_grads(a, gs[0])
    oa.step()
    assert oa.state[a[0]]["exp_avg"].dtype == torch.float32
    b = [p.detach().clone().requires_grad_(True) for p in a]
    ob = fused(b)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    for p, q in zip(a, b):
        for k in ("exp_avg", "exp_avg_sq"):
            assert ob.state[q][k].dtype == BF16 and torch.equal(ob.state[q][k], oa.state[p][k].to(BF16)), k
    set_grads(b, gs[1])
    ob.step()
    for i, (p, q) in enumerate(zip(a, b)):
        start = (p.detach().cpu(), gs[1][i], oa.state[p]["exp_avg"].to(BF16).cpu(),
                 oa.state[p]["exp_avg_sq"].to(BF16).cpu())
        check_against_chain((q.detach(), ob.state[q]["exp_avg"], ob.state[q]["exp_avg_sq"]), start, 2, LR,
                            what=f"after the fp32 checkpoint [{i}]")


# ------------------------------------------------------------------ refusals, each before any write
GUARD = 3.0


def guarded(n, dtype):
    return torch.full((n,), GUARD, dtype=dtype, device=DEV)


def untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t.float() == GUARD).all()) for t in ts)


def test_python_refusals_write_nothing():
    n = 40
    kw = dict(step=1, lr=LR, betas=C.BETAS, eps=C.EPS, weight_decay=WD)
    p, g, m, v = (guarded(n, BF16) for _ in range(4))
    p32, g32, master = guarded(n, torch.float32), guarded(n, torch.float32), guarded(n, torch.float32)
    with pytest.raises(ValueError, match="tensor 1: bfloat16 exp_avg / exp_avg_sq need a bfloat16 parameter"):
        P.adamw_step([p, p32], [g, g.clone()], [m, m.clone()], [v, v.clone()], **kw)
    with pytest.raises(ValueError, match="tensor 0: bfloat16 exp_avg / exp_avg_sq need a bfloat16 parameter"):
        P.adamw_step([p], [g32], [m], [v], **kw)
    with pytest.raises(ValueError, match="tensor 0: bfloat16 exp_avg / exp_avg_sq take no master"):
        P.adamw_step([p], [g], [m], [v], masters=[master], **kw)
    both = guarded(2 * n - 1, BF16)
    with pytest.raises(ValueError, match="m and v alias"):  # the library's own check, at 2-byte extents
        P.adamw_step([p], [g], [both[:n]], [both[n - 1:]], **kw)
    assert untouched(p, g, m, v, p32, g32, master, both)
    # back to back at the 2-byte extent is no overlap (at a 4-byte extent it would be one)
    two = torch.zeros(2 * n, dtype=BF16, device=DEV)
    P.adamw_step([p], [g], [two[:n]], [two[n:]], **kw)
    torch.cuda.synchronize()
    assert bool((two != 0).all())  # m and v were written (a step of 1e-3 is below half an ulp of p = 3)

    w = torch.nn.Parameter(guarded(n, BF16))
    opt = fused([w])
    if hasattr(w, "grad_dtype"):  # newer torch pins .grad to the parameter's dtype unless told otherwise
        w.grad_dtype = None
    w.grad = g32
    with pytest.raises(ValueError, match="need a bfloat16 parameter and gradient"):
        opt.step()
    assert untouched(w.detach())


def call_ex(p, g, m, v, state_dtype, p_dtype=_lib.BF16, g_dtype=_lib.BF16, master=None, record=None, sched=None):
    import ctypes

    a = _lib.AdamwArgs()
    a.p_dtype, a.g_dtype, a.count = p_dtype, g_dtype, 1
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        setattr(a, name, (ctypes.c_void_p * 1)(t.data_ptr() if isinstance(t, torch.Tensor) else t))
    if master is not None:
        a.master = (ctypes.c_void_p * 1)(master.data_ptr())
    a.numel = (ctypes.c_int64 * 1)(p.numel())
    a.step, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = 1, LR, 0.9, 0.95, 1e-8, WD
    return _lib.load().trlx_adamw_step_ex(ctypes.byref(a), state_dtype, record, sched, _lib.stream_of(p))


def test_c_abi_refusals_launch_nothing():
    ERR_ARG, ERR_DTYPE = 5, 3
    lib = _lib.load()
    n = 40
    p, g, m, v = (guarded(n, BF16) for _ in range(4))
    p32, master = guarded(n, torch.float32), guarded(n, torch.float32)
    cases = [
        (call_ex(p32, g, m, v, _lib.BF16, p_dtype=_lib.F32), "bf16 state takes bf16 parameters"),
        (call_ex(p, p32, m, v, _lib.BF16, g_dtype=_lib.F32), "bf16 state takes bf16 parameters"),
        (call_ex(p, g, m, v, 2), "state dtype"),
        (call_ex(p, g, m, v, _lib.BF16, master=master), "takes no master"),
        (call_ex(p, g, m.data_ptr() + 1, v, _lib.BF16), "m not aligned"),
        (call_ex(p, g, m, m.data_ptr() + 16, _lib.BF16), "m and v alias"),
        (call_ex(p, g, m, v, _lib.BF16, record=p32.data_ptr() + 4), "record is not aligned"),
        (call_ex(p, g, m, v, _lib.BF16, sched=p32.data_ptr() + 4), "schedule record is not aligned"),
    ]
    codes = [rc for rc, _ in cases]
    assert codes[0] == codes[1] == codes[2] == ERR_DTYPE and all(rc == ERR_ARG for rc in codes[3:]), codes
    # the message of the last refusal is the library's current one
    assert "schedule record" in lib.trlx_last_error().decode()
    assert untouched(p, g, m, v, p32, master)
    # the fp32 state through the new entry is the old entry bit for bit
    ps, gs = C.make_problem([CHUNK + 3], 1, seed=88, p_dtype=BF16, g_dtype=BF16)
    outs = []
    for route in ("old", "ex"):
        dp, dg = ps[0].to(DEV), gs[0][0].to(DEV)
        dm, dv = torch.zeros(CHUNK + 3, device=DEV), torch.zeros(CHUNK + 3, device=DEV)
        if route == "old":
            P.adamw_step([dp], [dg], [dm], [dv], step=1, lr=LR, betas=(0.9, 0.95), eps=1e-8, weight_decay=WD)
        else:
            assert call_ex(dp, dg, dm, dv, _lib.F32) == 0
        outs.append((dp, dm, dv))
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(x, y)
