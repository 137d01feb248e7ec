"""Shared pieces of the bf16-state AdamW tests (test_adamw_bf16_state_cpu.py,
test_gpu_adamw_bf16_state.py).

bf16_chain_step restates the update of trlx_adamw_step_ex(state_dtype = TRLX_BF16) in torch CPU
ops: every op a separately rounded fp32 op (torch's CPU kernels do not contract across ops),
its result rounded to bf16 (`.to(bfloat16).float()`, round-to-nearest-even) wherever torch's
_single_tensor_adam writes a bf16 tensor:

    p = bf(p * decay)
    m = bf(m + w1 * (g - m))
    v = bf(v * b2);  v = bf(v + w2 * (g * g))
    d = bf(sqrt(v));  d = bf(d / sqrt_bc2);  d = bf(d + eps)
    p = bf(p + neg_step * (m / d))

The fp32 scalars are formed in float64 and rounded once, as the library forms them
(adamw_device_checks.scalars; power=pow_libm is the default mode's route).
"""
import torch

import adamw_device_checks as D


def bf(x):
    """Round an fp32 tensor to bf16 (RNE) and widen it again."""
    return x.to(torch.bfloat16).float()


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def step_scalars(step, lr, betas, eps, wd, alpha=0.0, power=D.pow_libm):
    """The nine fp32 scalars of update `step` (numpy float32)."""
    return D.scalars(int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), float(wd), float(alpha),
                     power=power)


def bf16_chain_step(p, g, m, v, step, lr, betas, eps, wd, scalars=None):
    """Update number `step` of bf16 CPU tensors p, g, m, v -> (p, m, v), bf16, nothing in place.
    scalars: the nine fp32 scalars (None: step_scalars of the arguments)."""
    s = step_scalars(step, lr, betas, eps, wd) if scalars is None else scalars
    decay, w1, b2, w2, neg_step, sqrt_bc2, eps32 = (_f32(x) for x in s[:7])
    p, g, m, v = (t.detach().cpu().float() for t in (p, g, m, v))
    p = bf(p * decay)
    m = bf(m + w1 * (g - m))
    v = bf(v * b2)
    v = bf(v + w2 * (g * g))
    d = bf(torch.sqrt(v))
    d = bf(d / sqrt_bc2)
    d = bf(d + eps32)
    p = bf(p + neg_step * (m / d))
    return p.to(torch.bfloat16), m.to(torch.bfloat16), v.to(torch.bfloat16)


def bf16_clip(g, coef):
    """The gradient a clipped step takes: coef (the record's fp32 value) rounded to bf16, the
    fp32 product rounded to bf16 — torch's g.mul_(coef) with a 0-d device tensor."""
    c = bf(_f32(coef))
    return bf(g.detach().cpu().float() * c).to(torch.bfloat16)


def bf16_polyak(target, p_new, alpha):
    """trlx_polyak_update's bf16 form from the stored p: both products rounded to bf16, then the sum."""
    a, b = _f32(alpha), _f32(1.0 - float(alpha))
    return bf(bf(a * p_new.detach().cpu().float()) + bf(b * target.detach().cpu().float())).to(torch.bfloat16)


def same_bits(a, b):
    """Element-wise: equal bit patterns, or NaN on both sides (a NaN's payload is not pinned)."""
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    assert a.dtype == b.dtype == torch.bfloat16 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return (a.view(torch.int16) == b.view(torch.int16)) | (torch.isnan(a) & torch.isnan(b))


def assert_same_bits(got, want, what=""):
    ok = same_bits(got, want)
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements differ, first at {i}: "
                             f"{float(got.reshape(-1)[i])!r} vs {float(want.reshape(-1)[i])!r}")


def ulp_report(got, want, start=None):
    """(share of elements that differ, largest difference in bf16 ulps).  The ulp is taken at the
    smaller of the two magnitudes (neighbours across a power of two count as one ulp, not half)
    or, where `start` is given, at |start| if that is larger: `start` is the value the update
    began from (m before lerp_, p before addcdiv_).  m + w·(g - m) can cancel to a result many
    binades below m; every rounding inside the op is then relative to m, and the result's own
    ulp measures nothing — the reason adamw_checks.compare scales m by its inputs."""
    import adamw_checks as C

    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    differ = ~same_bits(got, want)
    if got.numel() == 0 or not bool(differ.any()):
        return 0.0, 0.0
    g, w = got.double()[differ], want.double()[differ]
    at = torch.minimum(g.abs(), w.abs())
    if start is not None:
        at = torch.maximum(at, start.detach().cpu().reshape(-1).double()[differ].abs())
    ulps = (g - w).abs() / C.bf16_ulp(at)
    worst = float("inf") if not bool(torch.isfinite(ulps).all()) else float(ulps.max())
    return float(differ.double().mean()), worst
