"""The oracle of the fused value head's tests: two restatements of make_head(n_embd, 1)
(trlx/model/nn/ppo_models.py:216-222) on the CPU.

  (a) reference_bf16   torch's own bf16 nn.Sequential (Linear, ReLU, Linear) and its bf16 autograd
  (b) oracle_fp64      the same function in fp64 with the ONE bf16 rounding of z = h·W1ᵀ + b1 that
                       a bf16 Linear applies; its autograd treats the rounding as the identity

The tests bound the kernel's distance to (b) by what (a) itself achieves:
    max|kernel − (b)| <= 2 · max|(a) − (b)| + 1e-6 · max|(b)|
(the factor 2: a different fp32 summation order may flip a bf16 rounding of z that torch's order
did not), for the values and for each of the five gradients.
"""
import torch
from torch import nn

GRADS = ("dh", "dw1", "db1", "dw2", "db2")


def make_case(N, H, seed):
    """Seeded bf16 operands of a value head on N tokens, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16
    return dict(h=torch.randn(N, H, generator=g).to(bf),
                w1=(torch.randn(2 * H, H, generator=g) / H ** 0.5).to(bf),
                b1=(0.1 * torch.randn(2 * H, generator=g)).to(bf),
                w2=(torch.randn(1, 2 * H, generator=g) / (2 * H) ** 0.5).to(bf),
                b2=(0.1 * torch.randn(1, generator=g)).to(bf),
                dv=torch.randn(N, generator=g).to(bf))


def reference_module(w1, b1, w2, b2):
    """The reference's nn.Sequential with these parameters (names 0.weight, 0.bias, 2.weight, 2.bias)."""
    H = w1.shape[1]
    m = nn.Sequential(nn.Linear(H, 2 * H).bfloat16(), nn.ReLU().bfloat16(), nn.Linear(2 * H, 1).bfloat16())
    m.load_state_dict({"0.weight": w1, "0.bias": b1, "2.weight": w2.reshape(1, -1), "2.bias": b2.reshape(1)},
                      strict=True)
    return m


def reference_bf16(h, w1, b1, w2, b2, dv=None):
    """(a): values [N] bf16 and, with dv, the five gradients of torch's bf16 autograd."""
    m = reference_module(w1, b1, w2, b2)
    x = h.detach().clone().requires_grad_(dv is not None)
    out = m(x)
    res = {"values": out.detach().squeeze(-1)}
    if dv is not None:
        out.backward(dv.to(torch.bfloat16).reshape(out.shape))
        res.update(dh=x.grad, dw1=m[0].weight.grad, db1=m[0].bias.grad, dw2=m[2].weight.grad.reshape(-1),
                   db2=m[2].bias.grad.reshape(-1))
    return res


def round_bf16_ste(z):
    """bf16 rounding of an fp64 tensor whose gradient is the identity."""
    return z + (z.detach().float().to(torch.bfloat16).double() - z.detach())


def oracle_fp64(h, w1, b1, w2, b2, dv=None):
    """(b): values [N] fp64 and, with dv, the five fp64 gradients."""
    t = [x.detach().double().requires_grad_(dv is not None) for x in (h, w1, b1, w2.reshape(-1), b2.reshape(-1))]
    hd, w1d, b1d, w2d, b2d = t
    z = round_bf16_ste(hd @ w1d.t() + b1d)
    v = torch.relu(z) @ w2d + b2d
    res = {"values": v.detach()}
    if dv is not None:
        v.backward(dv.double().reshape(v.shape))
        res.update(dh=hd.grad, dw1=w1d.grad, db1=b1d.grad, dw2=w2d.grad, db2=b2d.grad)
    return res


def max_err(x, ref):
    return float((x.detach().double().cpu().reshape(-1) - ref.double().reshape(-1)).abs().max())


def bound(e_ref, ref):
    return 2.0 * e_ref + 1e-6 * float(ref.double().abs().max())
