"""Shared by the CPU and GPU tests of the T5 RMSNorm with residual add (t5_rmsnorm / t5_add_rmsnorm):
the float64 oracle, HF's op sequence in the input dtype ("eager"), the seeded cases, a single-rounding
fp32 restatement of the kernel with six wrong variants, and the per-element rule

    |got - ref| <= ulp_dtype(|ref|) + 2^-16 * M
    M_y  = |w hh|                                     hh = h rstd
    M_dh = rstd (|g| + |hh| mean_j |g hh|) + |dh_in|  g = w dy
    M_dw = sum_n |dy hh|

ref: float64 (autograd for the gradients) of the inputs as stored, with h formed in float64 from the
dtype-rounded sum residual + x.  ulp_bf16(x) = 2^(floor(log2 x) - 7), ulp_f32(x) = 2^(floor(log2 x) - 23),
the exponent held at -126.  One ulp is the single rounding plus fp32 error; 2^-16 is 256 fp32 epsilons
for the fp32 reductions, good while no sequential fp32 addition chain exceeds about 128 terms.  The
kernel's chains: a thread's share of a row (at most 32 terms), 6 shuffle steps and 4 waves for a row
sum; for dw the rows one thread walks (N / (rows per workgroup pass x G), below 8 at every size the
tests use and 32 at the largest benchmarked shape), 4 waves, then 32 + 32 terms in the finish kernel:
under 128, so the constant stands as it is."""
import math

import torch

OUTPUTS = ("y", "dh", "dw")
EPS = 1e-6
WRONG = ("layernorm", "eps_outside", "dh_no_w", "dh_no_projection", "dw_no_rstd", "unrounded_sum")


# ------------------------------------------------------------------ cases
def case(N, D, dtype, seed=0, special=True):
    """residual ~ 3 N(0, 1) + 0.5 and x ~ N(0, 1) (h = residual + x has a nonzero mean), w ~ 1 + 0.3 N(0, 1),
    dy, dh_in ~ N(0, 1), rounded to dtype, on the CPU.  special: every fifth row from row 1 is scaled
    by 1e-3 (eps matters there) and the last row is all zero, as far as N reaches."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + D)
    residual = 3.0 * torch.randn(N, D, generator=g) + 0.5
    x = torch.randn(N, D, generator=g)
    w = 1.0 + 0.3 * torch.randn(D, generator=g)
    dy = torch.randn(N, D, generator=g)
    dh_in = torch.randn(N, D, generator=g)
    if special:
        residual[1::5] *= 1e-3
        x[1::5] *= 1e-3
        if N > 2:
            residual[-1] = 0.0
            x[-1] = 0.0
    return {k: t.to(dtype) for k, t in dict(x=x, residual=residual, w=w, dy=dy, dh_in=dh_in).items()}


def rounded_sum(c):
    """h as the kernel and torch form it: residual + x rounded once to the dtype."""
    return c["residual"] + c["x"]


# ------------------------------------------------------------------ float64
def norm64(h, w, eps=EPS, variant=None):
    """HF T5LayerNorm's expression in float64 (or a wrong forward)."""
    if variant == "layernorm":
        hc = h - h.mean(-1, keepdim=True)
        return w * (hc * torch.rsqrt(hc.pow(2).mean(-1, keepdim=True) + eps))
    if variant == "eps_outside":
        return w * (h / (torch.sqrt(h.pow(2).mean(-1, keepdim=True)) + eps))
    return w * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps))


def oracle(h, w, dy, dh_in=None, eps=EPS, variant=None):
    """{"y", "dh", "dw", "rstd"} in float64 from h (already the rounded sum), w, dy, dh_in as stored."""
    h64 = h.detach().double().requires_grad_()
    w64 = w.detach().double().requires_grad_()
    y = norm64(h64, w64, eps, variant if variant in ("layernorm", "eps_outside") else None)
    dh, dw = torch.autograd.grad(y, [h64, w64], dy.detach().double())
    hd, wd, g = h64.detach(), w64.detach(), dy.detach().double()
    rstd = torch.rsqrt(hd.pow(2).mean(-1, keepdim=True) + eps)
    hh = hd * rstd
    if variant == "dh_no_w":
        dh = rstd * (g - hh * (g * hh).mean(-1, keepdim=True))
    elif variant == "dh_no_projection":
        dh = rstd * (wd * g)
    elif variant == "dw_no_rstd":
        dw = (g * hd).sum(0)
    if dh_in is not None:
        dh = dh + dh_in.detach().double()
    return {"y": y.detach(), "dh": dh, "dw": dw, "rstd": rstd.squeeze(-1)}


def factors(h, w, dy, dh_in=None, eps=EPS):
    """M of the rule for each output, float64."""
    h, w, dy = h.double(), w.double(), dy.double()
    rstd = torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    hh = h * rstd
    g = w * dy
    M_dh = rstd * (g.abs() + hh.abs() * (g * hh).abs().mean(-1, keepdim=True))
    if dh_in is not None:
        M_dh = M_dh + dh_in.double().abs()
    return {"y": (w * hh).abs(), "dh": M_dh, "dw": (dy * hh).abs().sum(0)}


# ------------------------------------------------------------------ HF's op sequence in the input dtype
def hf_norm(h, w, eps=EPS):
    """transformers' T5LayerNorm.forward, op for op."""
    variance = h.to(torch.float32).pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(variance + eps)
    if w.dtype in (torch.float16, torch.bfloat16):
        h = h.to(w.dtype)
    return w * h


def eager(h, w, dy, dh_in=None, eps=EPS):
    """HF's module's op sequence and its autograd, every op rounded to the tensors' dtype."""
    hl, wl = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    y = hf_norm(hl, wl, eps)
    dh, dw = torch.autograd.grad(y, [hl, wl], dy)
    if dh_in is not None:
        dh = dh + dh_in
    return {"y": y.detach(), "dh": dh, "dw": dw}


# ------------------------------------------------------------------ the rule
def ulp(x, dtype):
    """The spacing of dtype at |x| (float64 in and out); 0 at 0."""
    bits = {torch.bfloat16: 7, torch.float32: 23}[dtype]
    x = x.abs().double()
    _, e = torch.frexp(x)
    e = torch.clamp(e - 1, min=-126)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - bits), torch.zeros_like(x))


def ratio(got, ref, M, dtype):
    """max over the elements of |got - ref| / (ulp(|ref|) + 2^-16 M); where the bound is 0 the element
    must be exact.  A non-finite `got` against a finite ref is inf."""
    got, ref = got.double().cpu(), ref.double().cpu()
    lim = ulp(ref, dtype) + 2.0 ** -16 * M.double().cpu()
    err = (got - ref).abs()
    r = torch.where(lim > 0, err / lim, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isfinite(got) | ~torch.isfinite(ref), r, torch.full_like(r, math.inf))
    r = torch.nan_to_num(r, nan=math.inf)
    return float(r.max()) if r.numel() else 0.0


def judge(got, want, M, dtype):
    """{output: worst ratio to the rule} for the outputs present in both."""
    return {n: ratio(got[n], want[n], M[n], dtype) for n in OUTPUTS if n in want and got.get(n) is not None}


# ------------------------------------------------------------------ a single-rounding fp32 restatement, and wrong ones
def restated(c, eps=EPS, wrong=None, dh_in=True):
    """The kernel's arithmetic restated on the CPU for the add form of case c: h the rounded sum, fp32
    throughout, every output rounded once.  {"h", "y", "dh", "dw"}.  wrong: None or one of WRONG --
    (i) a mean-subtracting LayerNorm, (ii) eps added outside the root, (iii) dh without w in g, (iv) dh
    without the projection term hh c, (v) dw without rstd (those five in float64, so that only the
    named mistake separates them from the oracle), (vi) the norm taken from the unrounded fp32 sum."""
    dtype = c["x"].dtype
    h = rounded_sum(c)
    din = c["dh_in"] if dh_in else None
    if wrong is not None and wrong != "unrounded_sum":
        o = oracle(h, c["w"], c["dy"], din, eps, variant=wrong)
        return {"h": h, **{n: o[n].to(dtype) for n in OUTPUTS}}
    f = torch.float32
    hf = h.to(f) if wrong is None else c["residual"].to(f) + c["x"].to(f)
    w, dy = c["w"].to(f), c["dy"].to(f)
    rstd = 1.0 / torch.sqrt(hf.pow(2).sum(-1, keepdim=True) / hf.shape[-1] + torch.tensor(eps, dtype=f))
    y = w * (hf * rstd)
    hh = hf * rstd
    g = w * dy
    cc = (g * hh).sum(-1, keepdim=True) / hf.shape[-1]
    dh = rstd * (g - hh * cc)
    if din is not None:
        dh = dh + din.to(f)
    dw = (dy * hh).sum(0)
    return {"h": h, "y": y.to(dtype), "dh": dh.to(dtype), "dw": dw.to(dtype)}
