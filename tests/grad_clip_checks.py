"""Shared pieces of the gradient-clipping tests (test_grad_clip_host.py, test_gpu_grad_clip.py).

The fp64 restatement of torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2.0):

  norm = sqrt(Σ over all tensors Σ g²)           in float64
  coef = min(max_norm / (norm + 1e-6), 1)        in float64
  g'   = g · coef                                in float64; a bf16 gradient is rounded back to
                                                 bf16, as the in-place multiply leaves it

(On the device torch applies the coefficient to a bf16 gradient rounded to bf16 first — a 0-d
device tensor is cast to the gradient's dtype — where torch on the CPU, and this restatement, keep
it in full: the GPU tests check the bf16 values bit for bit against torch on the device and
compare against this oracle with fp32 gradients only.)

followed by adamw_checks' float64 AdamW (oracle_run / oracle_one_step) on g'.  Results are
measured against it with adamw_checks.compare and accepted by adamw_checks.accepted
(e_fused <= 2 * e_torch, e_torch being torch's own clip_grad_norm_ + fp32 AdamW).

make_clip_problem scales the gradients of alternate steps so that the clip is active on the odd
steps (norm about twice max_norm, and small enough for the 1e-6 of the coefficient to matter)
and idle on the even ones (norm a fifth of max_norm: an unclamped coefficient would scale up).
"""
import math

import torch

import adamw_checks as C

MAX_NORM = 2e-3
STEP_SCALES = (1e-4, 1e-5)  # times a base norm of about 47: 5e-3 (clipped), 5e-4 (not clipped)


def make_clip_problem(sizes, steps, seed, g_dtypes=None):
    """Seeded N(0,1) fp32 parameters and per step gradients N(0,1) · 10^U{-1..0} (per element,
    fixed over the steps) · STEP_SCALES[k % 2], stored in g_dtypes[i] (default fp32)."""
    g_dtypes = g_dtypes or [torch.float32] * len(sizes)
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in sizes]
    scales = [10.0 ** torch.randint(-1, 1, (n,), generator=g).float() for n in sizes]
    grads = [[(torch.randn(n, generator=g) * s * STEP_SCALES[k % 2]).to(dt) for n, s, dt in zip(sizes, scales, g_dtypes)]
             for k in range(steps)]
    return params, grads


def norm64(grads):
    """sqrt(Σ g²) over a list of tensors in float64 on the CPU, as a Python float."""
    return math.sqrt(sum(float((g.detach().double().cpu() ** 2).sum()) for g in grads))


def clip64(grads, max_norm):
    """(norm, coef, [g' as float64 CPU tensors]) of one list of gradients."""
    norm = norm64(grads)
    coef = min(max_norm / (norm + 1e-6), 1.0) if math.isfinite(max_norm) else 1.0
    out = []
    for g in grads:
        s = g.detach().double().cpu() * coef
        out.append(s.to(torch.bfloat16).double() if g.dtype == torch.bfloat16 else s)
    return norm, coef, out


def oracle_run_clipped(params, grads, weight_decay, max_norm):
    """adamw_checks.oracle_run on the gradients clipped in float64, step by step."""
    return C.oracle_run(params, [clip64(gs, max_norm)[2] for gs in grads], weight_decay)


def oracle_one_step_clipped(p, g, m, v, step, lr, weight_decay, max_norm, all_grads=None):
    """One clipped update of one tensor in float64; the norm is taken over all_grads (default: g alone)."""
    _, coef, _ = clip64(all_grads if all_grads is not None else [g], max_norm)
    gs = g.detach().double().cpu() * coef
    if g.dtype == torch.bfloat16:
        gs = gs.to(torch.bfloat16).double()
    return C.oracle_one_step(p, gs, m, v, step, lr, weight_decay)


class ClippedAdamW(torch.optim.AdamW):
    """torch's route: torch.nn.utils.clip_grad_norm_ over every parameter, then AdamW.step()."""

    def __init__(self, params, max_norm, **kw):
        super().__init__(params, **kw)
        self.max_norm = max_norm

    def step(self, closure=None):
        torch.nn.utils.clip_grad_norm_([p for g in self.param_groups for p in g["params"]], self.max_norm)
        return super().step(closure)


def f32_ulp(x):
    """The spacing of float32 at |x| (a Python float; 24 significant bits)."""
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)
