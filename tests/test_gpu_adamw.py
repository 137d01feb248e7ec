"""Fused AdamW on the GPU (trlx_adamw_step, FusedAdamW, adamw_step, ILQLHeads.step_and_sync).

Accuracy is measured, not toleranced: ten steps under CosineAnnealingLR (1e-3 -> 1e-4 over 10),
betas (0.9, 0.95), eps 1e-8, against torch.optim.AdamW in float64 on the CPU; the kernel passes
when its error is at most twice that of torch's own fp32 AdamW on the device (default
implementation), for each of p, m, v as adamw_checks.compare defines them.
TRLX_ADAMW_PARITY_OUT=<file>: the measured figures are written there
(profiles/adamw_parity.json is such a run).

Sizes are the smallest that reach each path: 0, 1, 3, 7 elements, one below / at / above one
workgroup's chunk (_lib.ADAMW_CHUNK), more than one chunk, a list one longer than the table.
"""
import copy
import json
import os

import pytest
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import adamw_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = _lib.ADAMW_CHUNK
SIZES = [0, 1, 3, 7, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 13]
STEPS = 10
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    yield
    path = os.environ.get("TRLX_ADAMW_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "e_fused <= 2 * e_torch for each of p (units of lr 1e-3), m (relative to the "
                               "element's largest gradient), v (relative); e_* = max error against "
                               "torch.optim.AdamW in float64, e_torch = torch's fp32 AdamW on the device",
                       "cases": [dict(case=k, **_FIGURES[k]) for k in sorted(_FIGURES)]}, f, indent=1)


def torch_adamw(wd, **kw):
    return lambda ps: torch.optim.AdamW(ps, lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=wd, **kw)


def fused_adamw(wd, **kw):
    return lambda ps: P.FusedAdamW(ps, lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=wd, **kw)


def on_device(params, dtype=None):
    return [p.to(device=DEV, dtype=dtype or p.dtype).clone().requires_grad_(True) for p in params]


def check_rule(case, got, torch32, oracle, steps=None):
    """The acceptance rule at every step; the last step's figures are kept for the parity file."""
    for k in steps or range(len(oracle)):
        e_fused = C.compare(got[k]["p"], got[k]["m"], got[k]["v"], oracle[k])
        e_torch = C.compare(torch32[k]["p"], torch32[k]["m"], torch32[k]["v"], oracle[k])
        print(case, "step", k + 1, "e_fused", e_fused, "e_torch", e_torch)
        _FIGURES[case] = {"step": k + 1, "e_fused": e_fused, "e_torch": e_torch}
        assert C.accepted(e_fused, e_torch), (case, k + 1, e_fused, e_torch)


@pytest.fixture(scope="module")
def fp32_problem():
    """One problem per weight decay: the oracle and torch's fp32 device run are shared."""
    out = {}
    for wd in (0.0, 1e-2):
        params, grads = C.make_problem(SIZES, STEPS, seed=5)
        oracle = C.oracle_run(params, grads, wd)
        torch32 = C.run_optimizer(torch_adamw(wd), on_device(params), grads)
        out[wd] = (params, grads, oracle, torch32)
    return out


# ------------------------------------------------------------------ accuracy and sizes
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fp32_accuracy_over_ten_steps(fp32_problem, wd):
    """Every size of SIZES in one optimizer (numel 0, 1, 3, 7, chunk - 1, chunk, chunk + 1, > 2 chunks)."""
    params, grads, oracle, torch32 = fp32_problem[wd]
    got = C.run_optimizer(fused_adamw(wd), on_device(params), grads)
    check_rule(f"fp32 wd={wd}", got, torch32, oracle)


@pytest.mark.parametrize("size", SIZES[1:])
def test_each_size_alone_matches_the_list_run(fp32_problem, size):
    """A tensor's result does not depend on what else is in the table: bit-identical alone."""
    params, grads, _, _ = fp32_problem[1e-2]
    i = SIZES.index(size)
    both = C.run_optimizer(fused_adamw(1e-2), on_device(params), grads[:2])
    alone = C.run_optimizer(fused_adamw(1e-2), on_device([params[i]]), [[g[i]] for g in grads[:2]])
    lo = sum(SIZES[:i])
    for k in "pmv":
        assert torch.equal(alone[-1][k], both[-1][k][lo:lo + size]), k


def test_list_one_longer_than_the_table(fp32_problem):
    n = _lib.ADAMW_MAX_TENSORS + 1
    params, grads = C.make_problem([5 + (i % 3) for i in range(n)], 2, seed=6)
    oracle = C.oracle_run(params, grads, 1e-2)
    torch32 = C.run_optimizer(torch_adamw(1e-2), on_device(params), grads)
    got = C.run_optimizer(fused_adamw(1e-2), on_device(params), grads)
    check_rule("33 tensors", got, torch32, oracle)


@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
def test_fp32_parameter_with_either_gradient_dtype(g_dtype):
    """The functional form: fp32 p with fp32 / bf16 g (the bf16 values are the oracle's inputs)."""
    sizes = [7, CHUNK + 1]
    params, grads = C.make_problem(sizes, 3, seed=7, g_dtype=g_dtype)
    oracle = C.oracle_run(params, grads, 1e-2)
    torch32 = C.run_optimizer(torch_adamw(1e-2), on_device(params), [[g.float() for g in gs] for gs in grads])
    ps = [p.to(DEV) for p in params]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    got = []
    for step, (lr, gs) in enumerate(zip(C.cosine_lrs(3), grads), start=1):
        P.adamw_step(ps, [g.to(DEV) for g in gs], ms, vs, step=step, lr=lr, betas=C.BETAS, eps=C.EPS,
                     weight_decay=1e-2)
        got.append({"p": torch.cat(ps).double().cpu(), "m": torch.cat(ms).double().cpu(),
                    "v": torch.cat(vs).double().cpu()})
    check_rule(f"functional g={g_dtype}", got, torch32, oracle)


# ------------------------------------------------------------------ phases
SENTINEL = 12345.0


def phased(t, offset, pad=24):
    """A copy of `t` as a view at element `offset` of a larger sentinel-filled buffer."""
    buf = torch.full((t.numel() + pad,), SENTINEL, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()]
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("p_dtype, g_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                               (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("offsets", [(0, 1, 2, 3, 5, 6), (1, 1, 1, 1, 1, 1), (3, 7, 3, 3, 3, 3), (4, 4, 0, 4, 8, 12)])
@pytest.mark.parametrize("n", [5, CHUNK + 11])
def test_any_phase_gives_the_aligned_bits_and_touches_nothing_else(p_dtype, g_dtype, offsets, n):
    """p, g, m, v, master, target as views at the given element offsets of larger buffers: in
    fp32 (0, 1, 2, 3) puts each on another 16-B phase, in bf16 on another 2-B offset; all-ones
    is a shared phase with a head; (3, 7, 3, 3, 3, 3) a bf16 / fp32 pair that agrees modulo 4
    only.  The results are the bits of the aligned run, and every element outside the views keeps
    its sentinel."""
    params, grads = C.make_problem([n], 1, seed=8, p_dtype=p_dtype, g_dtype=g_dtype)
    g = torch.Generator().manual_seed(9)
    m0, v0 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    tgt0 = torch.randn(n, generator=g).to(p_dtype)
    with_master = p_dtype == torch.bfloat16
    base = [params[0], grads[0][0], m0, v0, params[0].float() + 1e-4 * m0, tgt0]
    kw = dict(step=3, lr=1e-3, betas=C.BETAS, eps=C.EPS, weight_decay=1e-2)

    def run(offs):
        bufs, views = zip(*[phased(t, o) for t, o in zip(base, offs)])
        p, gr, m, v, master, tgt = views
        P.adamw_step([p], [gr], [m], [v], masters=[master] if with_master else None, polyak=([tgt], [p], 0.25), **kw)
        torch.cuda.synchronize()
        return bufs, views

    _, want = run((0,) * 6)
    bufs, got = run(offsets)
    for name, w, x, buf, t0, off in zip("p g m v master target".split(), want, got, bufs, base, offsets):
        assert torch.equal(w, x), name
        assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all()), name
    assert torch.equal(got[1].cpu(), base[1])  # the gradient is read only
    if not with_master:
        assert torch.equal(got[4].cpu(), base[4])  # no master passed: untouched
    assert not torch.equal(got[0].cpu(), base[0]) and not torch.equal(got[5].cpu(), base[5])


# ------------------------------------------------------------------ bf16
def test_bf16_with_master_tracks_the_fp32_rule():
    """p is master.to(bfloat16) bit for bit after every step; the master meets the fp32 rule
    (oracle and torch's fp32 run start from the bf16 values and take the bf16 gradients)."""
    sizes = [3, CHUNK + 1, 2 * CHUNK + 13]
    params, grads = C.make_problem(sizes, STEPS, seed=12, p_dtype=torch.bfloat16, g_dtype=torch.bfloat16)
    oracle = C.oracle_run(params, grads, 1e-2)
    torch32 = C.run_optimizer(torch_adamw(1e-2), on_device(params, torch.float32),
                              [[g.float() for g in gs] for gs in grads])

    def snap(opt, ps):
        for p in ps:
            assert torch.equal(p.detach(), opt.state[p]["master"].to(torch.bfloat16))
            assert set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq", "master"}
        return C.state_snapshot(opt, ps, p_key="master")

    got = C.run_optimizer(fused_adamw(1e-2, master_weights=True), on_device(params), grads, snapshot=snap)
    check_rule("bf16 master", got, torch32, oracle)


def test_bf16_without_master_is_within_one_ulp_step_by_step():
    """Each step from the kernel's own previous state: p within one bf16 ulp of the float64
    result (half an ulp from the single rounding plus the fp32 error); m and v, which stay fp32,
    within 1e-6 relative to gmax / v of that one step."""
    sizes = [7, CHUNK + 1]
    params, grads = C.make_problem(sizes, STEPS, seed=13, p_dtype=torch.bfloat16, g_dtype=torch.bfloat16)
    ps = on_device(params)
    opt = fused_adamw(1e-2)(ps)
    sched = CosineAnnealingLR(opt, C.T_MAX, eta_min=C.ETA_MIN)
    worst = 0.0
    for step, gs in enumerate(grads, start=1):
        before = [(p.detach().cpu().clone(),
                   opt.state[p]["exp_avg"].cpu().clone() if p in opt.state else torch.zeros(p.numel()),
                   opt.state[p]["exp_avg_sq"].cpu().clone() if p in opt.state else torch.zeros(p.numel()))
                  for p in ps]
        lr = opt.param_groups[0]["lr"]
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.step()
        sched.step()
        for p, g, (p0, m0, v0) in zip(ps, gs, before):
            assert "master" not in opt.state[p] and p.dtype == torch.bfloat16
            po, mo, vo = C.oracle_one_step(p0, g, m0, v0, step, lr, 1e-2)
            ulps = ((p.detach().double().cpu() - po).abs() / C.bf16_ulp(po)).max()
            worst = max(worst, float(ulps))
            assert float(ulps) <= 1.0, (step, float(ulps))
            m, v = opt.state[p]["exp_avg"].double().cpu(), opt.state[p]["exp_avg_sq"].double().cpu()
            gmax = torch.maximum(g.double().abs(), m0.double().abs())
            assert float(((m - mo).abs() / gmax.clamp_min(1e-30)).max()) < 1e-6
            assert float(((v - vo).abs() / vo.clamp_min(1e-30)).max()) < 1e-6
    print("bf16 without master: worst distance", worst, "bf16 ulp")
    _FIGURES["bf16 no master"] = {"worst_ulp": worst, "bound_ulp": 1.0}


# ------------------------------------------------------------------ folded sync
def clone_setup(params, make_opt):
    ps = on_device(params)
    return ps, make_opt(ps)


@pytest.mark.parametrize("dtype, master", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True)])
@pytest.mark.parametrize("alpha", [0.001, 1.0])
def test_folded_sync_is_step_then_polyak_update_bit_for_bit(dtype, master, alpha):
    sizes = [1, 7, CHUNK + 1, 33, 64]  # the last two carry no gradient: plain Polyak, no step
    params, grads = C.make_problem(sizes, 3, seed=14, p_dtype=dtype, g_dtype=dtype)
    tg = torch.Generator().manual_seed(15)
    targets0 = [torch.randn(n, generator=tg).to(dtype) for n in sizes]
    results = []
    for folded in (True, False):
        ps, opt = clone_setup(params, fused_adamw(1e-2, master_weights=master))
        targets = [t.to(DEV).clone() for t in targets0]
        sources = [p.data for p in ps]
        for gs in grads:
            for p, g in zip(ps[:3], gs):
                p.grad = g.to(DEV)
            if folded:
                opt.step(polyak=(targets, sources, alpha))
            else:
                opt.step()
                P.polyak_update(targets, sources, alpha)
        torch.cuda.synchronize()
        results.append((ps, opt, targets))
    (pa, oa, ta), (pb, ob, tb) = results
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()), i
        sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
        assert set(sa) == set(sb) and bool(sa) == (i < 3)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, k)
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert torch.equal(a, b), i
        if dtype == torch.float32:  # (a bf16 target may round back to itself at alpha 0.001)
            assert not torch.equal(a.cpu(), targets0[i])
    for p, p0 in zip(pa[3:], params[3:]):  # no gradient: not stepped, no state
        assert torch.equal(p.detach().cpu(), p0) and p not in oa.state
    if alpha == 1.0:
        for t, p in zip(ta, pa):
            assert torch.equal(t, p.detach())


def test_ilql_heads_step_and_sync():
    """ILQLHeads.step_and_sync(opt) leaves what opt.step() then sync_target_q_heads() leaves."""
    torch.manual_seed(0)
    cfg = P.ILQLConfig()
    proto = P.ILQLHeads(cfg, 16, 37)
    g = torch.Generator().manual_seed(16)
    grads = {n: torch.randn(p.shape, generator=g) for n, p in proto.named_parameters() if p.requires_grad}
    out = []
    for folded in (True, False):
        heads = copy.deepcopy(proto).to(DEV)
        opt = P.FusedAdamW([p for p in heads.parameters() if p.requires_grad], lr=1e-2, betas=C.BETAS)
        for _ in range(2):
            for n, p in heads.named_parameters():
                if p.requires_grad:
                    p.grad = grads[n].to(DEV)
            if folded:
                heads.step_and_sync(opt)
            else:
                opt.step()
                heads.sync_target_q_heads()
        out.append({k: v.clone() for k, v in heads.state_dict().items()})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
        assert not torch.equal(out[0][k].cpu(), proto.state_dict()[k]), k


# ------------------------------------------------------------------ special values
def functional_state(n, seed, p_dtype=torch.float32):
    params, grads = C.make_problem([n], 1, seed=seed, p_dtype=p_dtype)
    p = params[0].to(DEV)
    return p, grads[0][0].to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)


KW = dict(betas=C.BETAS, eps=C.EPS)


def test_zero_gradient_changes_p_by_the_decay_only():
    p, g, m, v = functional_state(CHUNK + 3, 17)
    p0 = p.clone()
    P.adamw_step([p], [torch.zeros_like(g)], [m], [v], step=1, lr=1e-3, weight_decay=1e-2, **KW)
    assert bool((v == 0).all()) and bool((m == 0).all())
    assert torch.equal(p, p0 * (1 - 1e-3 * 1e-2)) and not torch.equal(p, p0)


def test_zero_learning_rate_leaves_p_and_advances_the_moments():
    p, g, m, v = functional_state(CHUNK + 3, 18)
    p0 = p.clone()
    P.adamw_step([p], [g], [m], [v], step=1, lr=0.0, weight_decay=1e-2, **KW)
    assert torch.equal(p, p0)
    torch.testing.assert_close(m, (1 - C.BETAS[0]) * g, rtol=1e-6, atol=0)
    torch.testing.assert_close(v, (1 - C.BETAS[1]) * g * g, rtol=1e-6, atol=0)


def test_inf_and_nan_gradients_poison_exactly_their_elements():
    n = CHUNK + 3
    p, g, m, v = functional_state(n, 19)
    clean = [t.clone() for t in (p, m, v)]
    P.adamw_step([clean[0]], [g], [clean[1]], [clean[2]], step=2, lr=1e-3, weight_decay=1e-2, **KW)
    bad = {5: float("inf"), n - 2: float("nan"), 4099: float("-inf")}
    for i, x in bad.items():
        g[i] = x
    P.adamw_step([p], [g], [m], [v], step=2, lr=1e-3, weight_decay=1e-2, **KW)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[list(bad)] = False
    for got, want in zip((p, m, v), clean):
        assert bool(torch.isfinite(want).all())
        assert torch.equal(got[keep], want[keep])
        assert not bool(torch.isfinite(got[~keep]).any())


# ------------------------------------------------------------------ interop with torch.optim.AdamW
def test_state_dict_moves_between_torch_and_fused_mid_run():
    """Three steps with one optimizer, its state_dict into the other, one more step: the fourth
    step meets the accuracy rule in both directions."""
    params, grads = C.make_problem([7, CHUNK + 1], 4, seed=20)
    oracle = C.oracle_run(params, grads, 1e-2)
    torch32 = C.run_optimizer(torch_adamw(1e-2), on_device(params), grads)
    for first, second, case in ((torch_adamw(1e-2), fused_adamw(1e-2), "torch -> fused"),
                                (fused_adamw(1e-2), torch_adamw(1e-2), "fused -> torch")):
        ps = on_device(params)
        a = first(ps)
        sched = CosineAnnealingLR(a, C.T_MAX, eta_min=C.ETA_MIN)
        for gs in grads[:3]:
            for p, g in zip(ps, gs):
                p.grad = g.to(DEV)
            a.step()
            sched.step()
        b = second(ps)
        b.load_state_dict(a.state_dict())
        assert b.param_groups[0]["lr"] == a.param_groups[0]["lr"] < C.LR_INIT
        for p, g in zip(ps, grads[3]):
            p.grad = g.to(DEV)
        b.step()
        assert all(float(b.state[p]["step"]) == 4.0 for p in ps)
        got = [None] * 3 + [C.state_snapshot(b, ps)]
        check_rule(case, got, torch32, oracle, steps=[3])


# ------------------------------------------------------------------ stream
def test_step_on_a_side_stream_needs_no_device_synchronise():
    """Tensors produced on a non-default stream and stepped there: the launch is ordered behind
    its producers on that stream (a launch on another stream would read them half-made)."""
    n = 4 * CHUNK + 5
    gen = torch.Generator().manual_seed(21)
    a = torch.randn(1024, 1024, generator=gen).to(DEV)
    p0 = torch.randn(n, generator=gen).to(DEV)
    torch.cuda.synchronize()

    def produce_and_step():
        x = a
        for _ in range(20):  # a few hundred microseconds of producer work in front of the step
            x = torch.tanh(x @ a * 1e-2)
        g = x.reshape(-1)[:n].contiguous()
        p = torch.nn.Parameter(p0 + x.reshape(-1)[n:2 * n] * 0)
        p.grad = g
        opt = P.FusedAdamW([p], lr=1e-3, betas=C.BETAS, weight_decay=1e-2)
        opt.step()
        return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]

    want = [t.clone() for t in produce_and_step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = produce_and_step()
        host = [t.cpu() for t in got]  # the copy is ordered on the side stream; no device sync
    for w, h in zip(want, host):
        assert torch.equal(w.cpu(), h)
    assert bool(host[1].abs().sum() > 0)
