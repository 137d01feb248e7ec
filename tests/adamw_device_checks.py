"""Shared pieces of the device-resident AdamW tests (test_adamw_device_host.py,
test_gpu_adamw_device.py).

The capturable mode forms b^step by a square-and-multiply product chain (trlx_adamw_advance in
include/trlx_t5_amd.h) where the default mode calls pow().  scalars() restates both routes in
Python floats and numpy.float32 roundings.  The GPU tests compare the two modes bit for bit, so
they run only on (betas, rates, weight decay, step range) tuples on which the two routes give
the same nine scalars: GPU_TUPLES below, asserted by the CPU suite.
"""
import math

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR

BETAS, EPS = (0.9, 0.95), 1e-8  # the reference's ppo_config.yml betas
LR_INIT, ETA_MIN, T_MAX = 1e-3, 1e-5, 10
N_UPDATES = 12
WEIGHT_DECAY = 1e-2
SCALAR_NAMES = ("decay", "w1", "b2", "w2", "neg_step", "sqrt_bc2", "eps", "alpha", "beta")


def pow_chain(b, n):
    """b**n as the library forms it: over the bits of n from the lowest, r = r*x where the bit
    is set, x = x*x while higher bits remain; every product one rounded float64 multiplication."""
    r, x, k = 1.0, float(b), int(n)
    while k:
        if k & 1:
            r = r * x
        if k >> 1:
            x = x * x
        k >>= 1
    return r


def pow_libm(b, n):
    """The default mode's route: the C library's pow on doubles."""
    return math.pow(float(b), float(n))


def scalars(step, lr, beta1, beta2, eps, weight_decay, alpha, power=pow_chain):
    """The nine fp32 scalars of update `step`: formed in float64, each rounded to float32 once."""
    bc1, bc2 = 1.0 - power(beta1, step), 1.0 - power(beta2, step)
    vals = (1.0 - lr * weight_decay, 1.0 - beta1, beta2, 1.0 - beta2, -(lr / bc1), math.sqrt(bc2), eps, alpha,
            1.0 - alpha)
    return np.array([np.float32(v) for v in vals], dtype=np.float32)


def same_bits(a, b):
    return bool((np.asarray(a, dtype=np.float32).view(np.uint32) == np.asarray(b, dtype=np.float32).view(np.uint32)).all())


def cosine(opt):
    return CosineAnnealingLR(opt, T_MAX, eta_min=ETA_MIN)


def cosine_rates(n=N_UPDATES):
    """The rates CosineAnnealingLR(T_MAX, ETA_MIN) from LR_INIT hands updates 1..n (plain floats)."""
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=LR_INIT)
    sched = cosine(opt)
    out = []
    for _ in range(n):
        out.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
    return out


# (betas, the rate of each update, weight decay, alpha of the folded sync, first step): every
# comparison of the capturable mode against the default mode on the GPU runs on one of these.
_COSINE = cosine_rates(N_UPDATES)
GPU_TUPLES = {
    "cosine12": (BETAS, _COSINE, WEIGHT_DECAY, 0.0, 1),              # bit equality with the host route
    "constant7": (BETAS, [LR_INIT] * 7, WEIGHT_DECAY, 0.25, 1),      # sync cadence against the host branch
    "table3of5": (BETAS, _COSINE[:3] + [_COSINE[2]] * 2, WEIGHT_DECAY, 0.0, 1),  # the last table entry holds
    "phase_step3": (BETAS, [_COSINE[2]], WEIGHT_DECAY, 0.25, 3),     # one clipped _dev launch at step 3
}
