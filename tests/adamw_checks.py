"""Shared pieces of the fused-AdamW tests (test_adamw_host.py, test_gpu_adamw.py).

The fp64 oracle is torch.optim.AdamW itself on float64 CPU copies (foreach=False), driven by the
same CosineAnnealingLR as the code under test.  compare() measures a result against it:

  p   max |p - p_oracle| / lr_unit — the error in units of the learning rate (one update moves
      an element by about lr, so this is the error relative to an update);
  m   max |m - m_oracle| / gmax, gmax the largest |gradient| the element has seen so far.  m is
      a convex combination of the element's past gradients (times the bias factor), so every
      rounding of its update is bounded by an ulp of gmax: this is m's relative error measured
      against the scale of its inputs.  Dividing by |m_oracle| itself instead would make the
      figure the luck of the one element whose 0.9·m + 0.1·g cancels most deeply, for torch's
      own fp32 route as much as for the kernel;
  v   max |v - v_oracle| / v_oracle — all of v's terms are non-negative, nothing cancels
      (an element whose oracle v is 0 must be 0).

The acceptance rule of the issue: e_fused <= 2 * e_torch for each of p, m, v, with e_torch
torch's own fp32 AdamW measured the same way (the margin of 2 covers a different order of the
same number of fp32 roundings per element per step).
"""
import math

import torch
from torch.optim.lr_scheduler import CosineAnnealingLR

LR_INIT, ETA_MIN, T_MAX = 1e-3, 1e-4, 10
BETAS, EPS = (0.9, 0.95), 1e-8


def make_problem(sizes, steps, seed, p_dtype=torch.float32, g_dtype=torch.float32):
    """Seeded N(0,1) parameters and, per step, gradients N(0,1) · 10^U{-4..2} with the exponent
    drawn per element once (an element keeps its scale over the steps).  CPU tensors of the
    requested dtypes: (params, [grads of step 1, ...])."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g).to(p_dtype) for n in sizes]
    scales = [10.0 ** torch.randint(-4, 3, (n,), generator=g).float() for n in sizes]
    grads = [[(torch.randn(n, generator=g) * s).to(g_dtype) for n, s in zip(sizes, scales)] for _ in range(steps)]
    return params, grads


def cosine_lrs(steps, lr=LR_INIT, eta_min=ETA_MIN, t_max=T_MAX):
    """The learning rate CosineAnnealingLR hands update 1, 2, ... (for the functional form)."""
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)
    sched = CosineAnnealingLR(opt, t_max, eta_min=eta_min)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


def run_optimizer(make_opt, params, grads, snapshot=None):
    """Drive an optimizer over `params` (leaf tensors) with CosineAnnealingLR: per step the
    gradients are set from grads[k], then opt.step(), scheduler.step().  Returns one
    {"p", "m", "v"} dict of flat CPU float64 tensors per step (all tensors concatenated)."""
    opt = make_opt(params)
    sched = CosineAnnealingLR(opt, T_MAX, eta_min=ETA_MIN)
    out = []
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.to(device=p.device, dtype=p.dtype)
        opt.step()
        sched.step()
        out.append(snapshot(opt, params) if snapshot else state_snapshot(opt, params))
    return out


def _flat(ts):
    return torch.cat([t.detach().reshape(-1).double().cpu() for t in ts]) if ts else torch.zeros(0, dtype=torch.float64)


def state_snapshot(opt, params, p_key=None):
    live = [p for p in params if p.numel()]
    return {"p": _flat([opt.state[p][p_key] if p_key else p for p in live]),
            "m": _flat([opt.state[p]["exp_avg"] for p in live]),
            "v": _flat([opt.state[p]["exp_avg_sq"] for p in live])}


def oracle_run(params, grads, weight_decay):
    """torch.optim.AdamW on float64 CPU copies, foreach=False.  Adds "gmax" (the largest
    |gradient| so far per element) to every step's record."""
    ps = [p.detach().double().cpu().clone().requires_grad_(True) for p in params]
    gs = [[g.double().cpu() for g in step] for step in grads]
    out = run_optimizer(lambda q: torch.optim.AdamW(q, lr=LR_INIT, betas=BETAS, eps=EPS, weight_decay=weight_decay,
                                                    foreach=False), ps, gs)
    gmax = None
    for rec, step in zip(out, gs):
        a = _flat(step).abs()
        gmax = a if gmax is None else torch.maximum(gmax, a)
        rec["gmax"] = gmax.clone()
    return out


def oracle_one_step(p, g, m, v, step, lr, weight_decay):
    """Update number `step` by torch.optim.AdamW in float64 from the given state: (p, m, v)."""
    q = p.detach().double().cpu().clone().requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=lr, betas=BETAS, eps=EPS, weight_decay=weight_decay, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.detach().double().cpu().clone(),
                    "exp_avg_sq": v.detach().double().cpu().clone()}
    q.grad = g.detach().double().cpu()
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


def compare(p, m, v, oracle, lr_unit=LR_INIT):
    """{"p", "m", "v"}: the errors of (p, m, v) (flat tensors) against one oracle record, as the
    module docstring defines them.  A non-finite value where the oracle is finite gives inf."""
    p, m, v = (t.detach().reshape(-1).double().cpu() for t in (p, m, v))

    def worst(err):
        if err.numel() == 0:
            return 0.0
        return float("inf") if not bool(torch.isfinite(err).all()) else float(err.max())

    def relative(x, xo, scale):  # scale 0: the value must be the oracle's
        err = (x - xo).abs()
        exact = torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf))
        return torch.where(scale > 0, err / scale.clamp_min(1e-300), exact)

    return {"p": worst((p - oracle["p"]).abs() / lr_unit), "m": worst(relative(m, oracle["m"], oracle["gmax"])),
            "v": worst(relative(v, oracle["v"], oracle["v"]))}


def accepted(e_fused, e_torch):
    """The acceptance rule: e_fused <= 2 * e_torch for each of p, m, v."""
    return all(e_fused[k] <= 2.0 * e_torch[k] for k in ("p", "m", "v"))


def bf16_ulp(x):
    """The spacing of bfloat16 at |x| (float64 tensor; 8 significant bits)."""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)
