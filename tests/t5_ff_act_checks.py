"""Shared by the CPU and GPU tests of the T5 feed-forward activation (t5_ff_act): the float64
oracle, HF's op sequence in the input dtype ("eager"), the seeded cases with their tail row, and
the per-element rule

    |got - ref| <= ulp_dtype(|ref|) + 2^-16 * M

ref: float64 (autograd for the gradients) of the inputs as stored.  ulp_bf16(x) = 2^(floor(log2 x) - 7),
ulp_f32(x) = 2^(floor(log2 x) - 23), the exponent held at the format's smallest normal one (-126).
M is the magnitude of the expression's factors: |u v| for y (|u| not gated), |dy v| for du (|dy| not
gated), |dy u| for dv.  One ulp is the single rounding (half an ulp at worst) plus fp32 error; the
floor covers the points where the derivative crosses zero (u ~ -0.75) and the deep negative tail,
where a relative bound means nothing; 2^-16 is 128 fp32 epsilons for about 16 fp32 operations
around one exp."""
import math

import torch

ACTS = ("relu", "gelu_new", "silu")
OUTPUTS = ("y", "du", "dv")
K = math.sqrt(2.0 / math.pi)
C = 0.044715
# the tail row of u; in the columns of the last three pairs v = dy = 1
TAIL = [0.0, -0.0, 1e-30, -1e-30, 0.75, -0.75, -0.7518, 3.0, -3.0, 6.0, -6.0, 10.0, -10.0, 12.0, -12.0, 20.0, -20.0,
        40.0, -40.0, 100.0, -100.0, 1e4, -1e4, 1e19, -1e19, 3e38, -3e38]
TAIL_ONES = 6


# ------------------------------------------------------------------ float64 oracle
def act64(u, act):
    """act(u) in float64 in a form autograd differentiates without 0 * inf: gelu_new as
    u * sigmoid(2 z), z = sqrt(2/pi) (u + 0.044715 u^3), which is 0.5 u (1 + tanh z)."""
    assert u.dtype == torch.float64
    if act == "relu":
        return torch.relu(u)
    if act == "silu":
        return u * torch.sigmoid(u)
    if act == "gelu_new":
        return u * torch.sigmoid(2.0 * K * (u + C * u * u * u))
    raise ValueError(act)


def oracle(u, v, dy, act):
    """{"y", "du", "dv"} in float64 from the inputs as stored (v None: not gated, no "dv")."""
    u64 = u.detach().double().requires_grad_()
    leaves = [u64]
    v64 = None
    if v is not None:
        v64 = v.detach().double().requires_grad_()
        leaves.append(v64)
    y = act64(u64, act)
    if v64 is not None:
        y = y * v64
    grads = torch.autograd.grad(y, leaves, dy.detach().double())
    out = {"y": y.detach(), "du": grads[0]}
    if v is not None:
        out["dv"] = grads[1]
    return out


# ------------------------------------------------------------------ HF's op sequence in the input dtype
def eager_act(u, act):
    if act == "gelu_new":   # transformers.activations.NewGELUActivation.forward
        return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * torch.pow(u, 3.0))))
    if act == "silu":
        return torch.nn.functional.silu(u)
    return torch.nn.functional.relu(u)


def eager(u, v, dy, act):
    """HF's modules' op sequence and its autograd, every op rounded to the tensors' dtype."""
    ug = u.detach().clone().requires_grad_()
    leaves = [ug]
    vg = None
    if v is not None:
        vg = v.detach().clone().requires_grad_()
        leaves.append(vg)
    y = eager_act(ug, act)
    if vg is not None:
        y = y * vg
    grads = torch.autograd.grad(y, leaves, dy)
    out = {"y": y.detach(), "du": grads[0]}
    if v is not None:
        out["dv"] = grads[1]
    return out


# ------------------------------------------------------------------ cases
def case(N, F, dtype, scale=1.0, gated=True, seed=0, tail=True):
    """u, v ~ N(0, 1) * scale, dy ~ N(0, 1), rounded to dtype, on the CPU.  The tail values of u go
    to the first elements in row-major order (row 0 when F >= len(TAIL)), as far as N * F reaches."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + F)
    u = torch.randn(N, F, generator=g) * scale
    v = torch.randn(N, F, generator=g) * scale
    dy = torch.randn(N, F, generator=g)
    if tail:
        n = min(len(TAIL), N * F)
        u.view(-1)[:n] = torch.tensor(TAIL[:n])
        lo = len(TAIL) - TAIL_ONES
        if n > lo:
            v.view(-1)[lo:n] = 1.0
            dy.view(-1)[lo:n] = 1.0
    u, v, dy = (t.to(dtype) for t in (u, v, dy))
    return {"u": u, "v": v if gated else None, "dy": dy}


# ------------------------------------------------------------------ the rule
def ulp(x, dtype):
    """The spacing of dtype at |x| (float64 in and out); 0 at 0."""
    bits = {torch.bfloat16: 7, torch.float32: 23}[dtype]
    x = x.abs().double()
    _, e = torch.frexp(x)                       # x = m 2^e, m in [0.5, 1): floor(log2 x) = e - 1
    e = torch.clamp(e - 1, min=-126)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - bits), torch.zeros_like(x))


def factors(u, v, dy):
    """M of the rule for each output, float64."""
    u, dy = u.double().abs(), dy.double().abs()
    if v is None:
        return {"y": u, "du": dy}
    v = v.double().abs()
    return {"y": u * v, "du": dy * v, "dv": dy * u}


def ratio(got, ref, M, dtype):
    """max over the elements of |got - ref| / (ulp(|ref|) + 2^-16 M); where the bound is 0 the
    element must be exact.  A non-finite `got` against a finite ref is inf."""
    got, ref = got.double().cpu(), ref.double().cpu()
    lim = ulp(ref, dtype) + 2.0 ** -16 * M.double().cpu()
    err = (got - ref).abs()
    r = torch.where(lim > 0, err / lim, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isfinite(got) | ~torch.isfinite(ref), r, torch.full_like(r, math.inf))
    r = torch.nan_to_num(r, nan=math.inf)
    return float(r.max()) if r.numel() else 0.0


def judge(got, want, u, v, dy, dtype):
    """{output: worst ratio to the rule} for the outputs present in both."""
    M = factors(u, v, dy)
    return {n: ratio(got[n], want[n], M[n], dtype) for n in OUTPUTS if n in want and got.get(n) is not None}


# ------------------------------------------------------------------ a single-rounding fp32 restatement, and wrong ones
def restated(u, v, dy, act, wrong=None):
    """The kernel's arithmetic restated on the CPU: fp32 throughout from e = exp(-|x|), every
    output rounded once to the inputs' dtype.  wrong: None, or one of
      "erf"       the erf GELU in place of gelu_new
      "silu"      silu in place of gelu_new
      "swapped"   act(v) * u
      "no_cubic"  the derivative of gelu_new without the 3 * 0.044715 u^2 term
    (the wrong ones in float64, so that only the named mistake separates them from the oracle)."""
    dtype = u.dtype
    if wrong is not None:
        w = torch.float64
        uu, vv, gg = u.to(w), None if v is None else v.to(w), dy.to(w)
        if wrong == "swapped":
            uu, vv = vv, uu
        x = uu if (act == "silu" or wrong == "silu") else 2.0 * K * (uu + C * uu ** 3)
        xp = torch.ones_like(uu) if (act == "silu" or wrong == "silu") else 2.0 * K * (1.0 + (0.0 if wrong == "no_cubic" else 3.0 * C) * uu * uu)
        s = torch.sigmoid(x)
        a, d = uu * s, s + uu * xp * s * (1.0 - s)
        if wrong == "erf":
            a = torch.nn.functional.gelu(uu)
            d = 0.5 * (1.0 + torch.erf(uu / math.sqrt(2.0))) + uu * torch.exp(-0.5 * uu * uu) / math.sqrt(2.0 * math.pi)
        out = {"y": a if vv is None else a * vv, "du": gg * d if vv is None else gg * vv * d}
        if vv is not None:
            out["dv"] = gg * a
            if wrong == "swapped":
                out["du"], out["dv"] = out["dv"], out["du"]
        return {n: t.to(dtype) for n, t in out.items()}
    f = torch.float32
    uu, vv, gg = u.to(f), None if v is None else v.to(f), dy.to(f)
    if act == "relu":
        a = torch.where(uu <= 0, torch.zeros_like(uu), uu)
        d = torch.where(uu > 0, torch.ones_like(uu), torch.where(uu <= 0, torch.zeros_like(uu), uu))
    else:
        if act == "silu":
            x, xp = uu, torch.ones_like(uu)
        else:
            u2 = uu * uu
            x = f32(2.0 * K) * (uu * (1.0 + f32(C) * u2))
            xp = f32(2.0 * K) * (1.0 + f32(3.0 * C) * u2)
        e = torch.exp(-x.abs())
        r = 1.0 / (1.0 + e)
        s = torch.where(x >= 0, r, e * r)
        a = uu * s
        t = e * (r * r)
        d = s + torch.where(t > 0, (uu * xp) * t, torch.zeros_like(t))
    out = {"y": a if vv is None else a * vv, "du": gg * d if vv is None else (gg * vv) * d}
    if vv is not None:
        out["dv"] = gg * a
    return {n: t.to(dtype) for n, t in out.items()}


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))
