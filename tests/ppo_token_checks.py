"""Shared pieces of the [B, T] PPO token-kernel tests (test_ppo_token_cpu.py, test_gpu_ppo_token.py):
token_rows.hip (KL reward, GAE scan, moments, whiten) and ppo_loss.hip (loss, finalize, scale_by).

Three things are compared on the same seeded inputs:
  *64   float64 restatements written here from the formulas (not calls into the oracle), pinned
        to the reference's fixtures by test_ppo_token_cpu.py;
  *32   oracle/ppo_oracle.py run in fp32 on the CPU: "torch in fp32";
  the kernel.

compare() gives max errors against the float64 result per output; accepted() is the rule

    e_kernel <= 2 * e_ref32   per output;
    where e_ref32 is exactly 0 the kernel may be off by one fp32 ulp of the output's largest
    magnitude instead.

An output is one buffer the kernel writes (the advantages, the whitened values, a gradient, the
stats vector with the loss as element 0), and its error is max |x - x64| over its elements.
Where the float64 result is NaN or infinite the value must be the same NaN / infinity, otherwise
the error is inf.  The stats vector is not measured per element or relatively: a stat such as
approx_kl = mean((ratio - 1) - log_ratio) cancels, so its error is the rounding noise of fp32
exp(), which the device and the CPU round independently; two such noises differ by more than a
factor of two about as often as not (measured on MI355X: relative errors 2.4e-7 against 1.1e-7 at
n = 512, 4.9e-7 against 1.5e-7 with bf16 operands), which says nothing about either side.  Each
stat is still held to RT32 against the fp32 oracle by the GPU tests.

bf16 outputs are compared with the float64 result rounded once to bf16, within one bf16 ulp
(bf16_close).  No assertion built on this file is looser than RT32 for an fp32 output.
"""
import math

import numpy as np
import torch

from oracle import ppo_oracle as orc

RT32 = dict(rtol=1e-5, atol=1e-5)
STATS_KEYS = ("losses/total_loss", "losses/policy_loss", "losses/value_loss",
              "values/mean_old_values", "values/var_old_values", "values/mean_values", "values/values_error",
              "values/clipfrac", "policy/approx_kl", "policy/clipfrac", "returns/mean", "returns/var", "ratio")
# (gamma, lam): the two the rest of the suite uses, then pairs whose fl32(fl32(g)*fl32(l)) is one ulp
# off fl32(g*l)
GL_PAIRS = [(1.0, 0.95), (0.99, 0.95), (0.99, 0.99), (0.98, 0.9), (0.95, 0.9), (0.9, 0.95), (0.995, 0.97)]


def f64(t):
    return None if t is None else t.detach().double().cpu()


# ------------------------------------------------------------------ float64 restatements
def pad_mask(lengths, T):
    """True where column t >= lengths[b] (store padding)."""
    return torch.arange(T)[None, :] >= lengths[:, None]


def kl_reward64(lp, ref_lp, beta, scores=None, lengths=None):
    """r = -beta (lp - ref_lp); the score is added on each row's last valid column; columns past
    the length are 0; a row of length 0 is all zeros."""
    lp, ref_lp = f64(lp), f64(ref_lp)
    B, T = lp.shape
    r = -float(beta) * (lp - ref_lp)
    ln = torch.full((B,), T, dtype=torch.int64) if lengths is None else lengths.cpu().long()
    r[pad_mask(ln, T)] = 0.0
    if scores is not None:
        rows = torch.arange(B)[ln > 0]
        r[rows, ln[rows] - 1] += f64(scores)[rows]
    return r


def gae64(values, rewards, Teff, gamma, lam, lengths=None, mask=None):
    """delta_t = r_t + gamma V_{t+1} - V_t (V_Teff = 0); A_t = delta_t + gamma lam A_{t+1}; returns
    = A + V over columns [0, Teff) of zero-padded inputs.  Returns (adv, ret, record) with record
    = [sum A, sum A^2, count, sum mask] (mask None: count)."""
    v, r = f64(values), f64(rewards)
    if lengths is not None:
        pad = pad_mask(lengths.cpu().long(), v.shape[1])
        v, r = v.masked_fill(pad, 0.0), r.masked_fill(pad, 0.0)
    v, r = v[:, :Teff], r[:, :Teff]
    B = v.shape[0]
    adv = torch.zeros(B, Teff, dtype=torch.float64)
    last = torch.zeros(B, dtype=torch.float64)
    gl = float(gamma) * float(lam)
    for t in range(Teff - 1, -1, -1):
        nxt = v[:, t + 1] if t + 1 < Teff else 0.0
        last = r[:, t] + float(gamma) * nxt - v[:, t] + gl * last
        adv[:, t] = last
    n = float(B * Teff)
    rec = torch.tensor([float(adv.sum()), float((adv * adv).sum()), n,
                        n if mask is None else float(mask.double().sum())], dtype=torch.float64)
    return adv, adv + v, rec


def moments64(x):
    """[sum, sum of squares, count, 0]; an int64 input is summed in Python integers (exact)."""
    x = x.detach().cpu().reshape(-1)
    if x.dtype == torch.int64:
        xs = [int(e) for e in x.tolist()]
        return [sum(xs), sum(e * e for e in xs), len(xs), 0]
    d = x.double()
    return [math.fsum(d.tolist()), math.fsum((d * d).tolist()), d.numel(), 0]


def whiten64(x, unbiased=True, shift_mean=True):
    """(x - mean) rsqrt(var + 1e-8) (+ mean); var = M2 / (n - 1) or M2 / n.  n = 1 unbiased: NaN."""
    d = f64(x)
    n = d.numel()
    mean = d.sum() / n
    m2 = ((d - mean) ** 2).sum()
    den = n - 1 if unbiased else n
    var = m2 / den if den > 0 else torch.tensor(float("nan"), dtype=torch.float64)
    out = (d - mean) / torch.sqrt(var + 1e-8)
    return out if shift_mean else out + mean


def ppo_loss64(lp, v, olp, ov, adv, ret, mask=None, c=0.2, cv=0.2, vf_coef=1.0, adv_stats=None, unbiased=True):
    """The clipped-surrogate + clipped-value loss with its 13 stats (STATS_KEYS order) and, through
    autograd, d loss / d lp and d loss / d v.  adv_stats = (sum, sumsq, n): the advantages are
    whitened first (var over n - 1 when unbiased).  Returns dict(stats [13], dlp, dv); stats[0]
    is the loss."""
    lp = f64(lp).clone().requires_grad_(True)
    v = f64(v).clone().requires_grad_(True)
    olp, ov, adv, ret = f64(olp), f64(ov), f64(adv), f64(ret)
    m = torch.ones_like(olp) if mask is None else f64(mask)
    if adv_stats is not None:
        s1, s2, n = (float(e) for e in adv_stats)
        mean = s1 / n
        var = (s2 - s1 * mean) / ((n - 1) if unbiased else n)
        adv = (adv - mean) / math.sqrt(var + 1e-8)
    N = olp.numel()
    msum = m.sum()
    vclip = torch.clamp(v, ov - cv, ov + cv)
    vl1, vl2 = (v - ret) ** 2, (vclip - ret) ** 2
    vf = 0.5 * (torch.maximum(vl1, vl2) * m).sum() / msum
    lr = (lp - olp) * m
    ratio = torch.exp(lr)
    pg1, pg2 = -adv * ratio, -adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)
    pg = (torch.maximum(pg1, pg2) * m).sum() / msum
    loss = pg + vf_coef * vf
    loss.backward()

    def var_of(x):  # torch.var: unbiased; N = 1 -> NaN
        return ((x - x.mean()) ** 2).sum() / (N - 1) if N > 1 else torch.tensor(float("nan"), dtype=torch.float64)

    with torch.no_grad():
        stats = torch.stack([
            loss, pg, vf, ov.mean(), var_of(ov), v.mean(), vl1.mean(), (vl2 > vl1).double().mean(),
            ((ratio - 1) - lr).mean(), (pg2 > pg1).double().mean(), ret.mean(), var_of(ret),
            (ratio * m).sum() / msum]).detach()
    return dict(stats=stats, dlp=lp.grad, dv=v.grad)


# ------------------------------------------------------------------ torch in fp32 (the oracle)
def kl_reward32(lp, ref_lp, beta, scores=None, lengths=None):
    return orc.kl_penalty_rewards(lp.float().cpu(), ref_lp.float().cpu(), beta,
                                  None if scores is None else scores.float().cpu(),
                                  None if lengths is None else lengths.cpu().long())


def gae32(values, rewards, Teff, gamma, lam, lengths=None):
    """The oracle's loop on fp32 copies (bf16 inputs: their exact fp32 values), unwhitened."""
    ln = None if lengths is None else lengths.cpu().long()
    v = orc.store_padded(values.float().cpu(), ln)[:, :Teff]
    r = orc.store_padded(rewards.float().cpu(), ln)[:, :Teff]
    return orc.gae(v, r, Teff, gamma, lam, use_whitening=False)


def whiten32(x, unbiased=True, shift_mean=True):
    """oracle.whiten (torch.var_mean) when unbiased; the biased branch is the oracle's
    global_statistics on one rank: the same two fp32 sums without the all-reduces."""
    xs = x.float().cpu()
    if unbiased:
        return orc.whiten(xs, shift_mean=shift_mean, distributed=False)
    mean = xs.sum() / xs.numel()
    var = torch.sum((xs - mean) ** 2) / xs.numel()
    out = (xs - mean) * torch.rsqrt(var + 1e-8)
    return out if shift_mean else out + mean


def ppo_loss32(lp, v, olp, ov, adv, ret, mask=None, c=0.2, cv=0.2, vf_coef=1.0, adv_stats=None, unbiased=True):
    lp = lp.float().cpu().clone().requires_grad_(True)
    v = v.float().cpu().clone().requires_grad_(True)
    olp, ov, adv, ret = (t.float().cpu() for t in (olp, ov, adv, ret))
    m = torch.ones(olp.shape, dtype=torch.long) if mask is None else mask.cpu().long()
    if adv_stats is not None:  # whiten, then loss (fp32; the biased form as in whiten32)
        adv = whiten32(adv, unbiased=unbiased)
    loss, st = orc.ppo_loss(lp, v, olp, ov, adv, ret, m, c, cv, vf_coef)
    loss.backward()
    stats = torch.stack([torch.as_tensor(st[k], dtype=torch.float32).detach() for k in STATS_KEYS])
    stats[0] = loss.detach()
    return dict(stats=stats, dlp=lp.grad, dv=v.grad)


# ------------------------------------------------------------------ measuring
def ulp32(x):
    """The fp32 spacing at |x|."""
    return float(np.spacing(np.float32(abs(float(x)))))


def _one(name, got, want):
    got, want = f64(got).reshape(-1), f64(want).reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.numel() == 0:
        return 0.0, 0.0
    fin = torch.isfinite(want)
    same_special = bool((torch.isnan(got) == torch.isnan(want)).all()) and bool((got[~fin & ~torch.isnan(want)]
                                                                                == want[~fin & ~torch.isnan(want)]).all())
    if not same_special or not bool(torch.isfinite(got[fin]).all()):
        return math.inf, 0.0
    g, w = got[fin], want[fin]
    if g.numel() == 0:
        return 0.0, 0.0
    return float((g - w).abs().max()), ulp32(w.abs().max())


def compare(got, want64):
    """{output: max error of got[output] against want64[output]} as the module docstring defines
    it, plus "_ulp": {output: the one-ulp allowance accepted() uses where the fp32 oracle is exact}."""
    out, ulps = {}, {}
    for k in want64:
        out[k], ulps[k] = _one(k, got[k], want64[k])
    out["_ulp"] = ulps
    return out


def accepted(e_kernel, e_ref32):
    """e_kernel <= 2 e_ref32 per output; one fp32 ulp where e_ref32 is exactly 0."""
    return all(e_kernel[k] <= (2.0 * e_ref32[k] if e_ref32[k] > 0 else e_kernel["_ulp"][k])
               for k in e_kernel if k != "_ulp")


def figures(e):
    return {k: v for k, v in e.items() if k != "_ulp"}


def bf16_ulp(x):
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def bf16_close(got, want64):
    """got (bf16) is within one bf16 ulp of want64 rounded once to bf16 (NaN where it is NaN)."""
    want = f64(want64).reshape(-1)
    g = f64(got).reshape(-1)
    w = want.to(torch.bfloat16).double()
    nan = torch.isnan(w)
    if not bool((torch.isnan(g) == nan).all()):
        return False
    return bool(((g - w).abs()[~nan] <= bf16_ulp(w[~nan])).all())


# ------------------------------------------------------------------ seeded inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def kl_inputs(B, T, seed, dtype=torch.float32):
    g = gen(seed)
    lp = (-torch.rand(B, T, generator=g) * 6).to(dtype)
    ref = (lp.float() + 0.3 * torch.randn(B, T, generator=g)).to(dtype)
    scores = torch.rand(B, generator=g) * 20 - 10
    return lp, ref, scores


def edge_lengths(B, T, seed):
    """Random lengths in [0, T] with 0, 1 and T planted (as far as B allows)."""
    ln = torch.randint(0, T + 1, (B,), generator=gen(seed))
    for i, val in enumerate((T, 1, 0)):
        if i < B:
            ln[(i * 7) % B if B > 21 else i] = min(val, T)
    return ln


def gae_inputs(B, T, seed, dtype=torch.float32):
    g = gen(seed)
    v = torch.randn(B, T, generator=g).to(dtype)
    r = (0.1 * torch.randn(B, T, generator=g)).to(dtype)
    return v, r


def loss_inputs(n, T, seed, mask="ones", bf16=()):
    """Six [B, T] operands (names in `bf16` are bf16, the rest fp32) and a mask: "ones", "random",
    "single" (one 1), or None."""
    g = gen(seed)
    B = n // T
    assert B * T == n
    olp = -torch.rand(B, T, generator=g) * 4
    d = dict(lp=olp + 0.15 * torch.randn(B, T, generator=g), olp=olp)
    d["ov"] = torch.randn(B, T, generator=g)
    d["v"] = d["ov"] + 0.3 * torch.randn(B, T, generator=g)
    d["adv"] = torch.randn(B, T, generator=g)
    d["ret"] = d["ov"] + 0.5 * torch.randn(B, T, generator=g)
    for k in bf16:
        d[k] = d[k].to(torch.bfloat16)
    if mask == "ones":
        m = torch.ones(B, T, dtype=torch.int64)
    elif mask == "random":
        m = (torch.rand(B, T, generator=g) < 0.7).long()
        m.view(-1)[0] = 1
    elif mask == "single":
        m = torch.zeros(B, T, dtype=torch.int64)
        m.view(-1)[(n * 2) // 3] = 1
    else:
        m = None
    d["mask"] = m
    return d


def _exp_hits(olp, bound):
    """lp (fp32) with fp32 exp(lp - olp) == bound exactly, or None: the neighbours of olp +
    log(bound) are tried and the middle hit is taken."""
    lp0 = np.float32(olp + np.float32(math.log(float(bound))))
    cand, x = [], np.nextafter(lp0, np.float32(-np.inf), dtype=np.float32)
    for _ in range(4):
        x = np.nextafter(x, np.float32(-np.inf), dtype=np.float32)
    for _ in range(10):
        if float(torch.exp(torch.tensor(np.float32(x - olp)))) == float(bound):
            cand.append(x)
        x = np.nextafter(x, np.float32(np.inf), dtype=np.float32)
    return cand[len(cand) // 2] if cand else None


def tie_inputs(n, seed, c=0.2, cv=0.2):
    """loss_inputs(n, 1, mask "ones") with exact fp32 ties and bounds planted in disjoint eighths
    of the positions (the bounds as the fp32 ops form them: ov -/+ fl32(cv), 1 -/+ fl32(c)):
      0 v == ov - cv    1 v == ov + cv    2 ratio == 1 - c    3 ratio == 1 + c    4 A == 0
      5 vl1 == vl2 with v outside the clip range (ret midway between v and the clipped v).
    Returns (inputs, planted) with planted[k] the positions where plant k took (a ratio plant
    takes only where an lp with fp32 exp(lp - olp) on the bound exists)."""
    d = loss_inputs(n, 1, seed)
    f32 = np.float32
    lo, hi = f32(1.0) - f32(c), f32(1.0) + f32(c)
    planted = {k: [] for k in range(6)}
    for i in range(n):
        k = i % 8
        ov, olp = f32(d["ov"][i, 0]), f32(d["olp"][i, 0])
        if k == 0:
            d["v"][i, 0] = float(ov - f32(cv))
        elif k == 1:
            d["v"][i, 0] = float(ov + f32(cv))
        elif k in (2, 3):
            lp = _exp_hits(olp, lo if k == 2 else hi)
            if lp is None:
                continue
            d["lp"][i, 0] = float(lp)
        elif k == 4:
            d["adv"][i, 0] = 0.0
        elif k == 5:  # on a 2^-8 grid so that the midpoint and both differences are exact
            ovq = f32(round(float(ov) * 256) / 256)
            v = ovq + f32(0.75)
            vc = ovq + f32(cv)  # the clipped value as fp32 forms it
            d["ov"][i, 0], d["v"][i, 0] = float(ovq), float(v)
            ret = f32((np.float64(v) + np.float64(vc)) / 2)  # may round: taken only where the tie holds
            d["ret"][i, 0] = float(ret)
            e1, e2 = v - ret, vc - ret
            if e1 * e1 != e2 * e2:
                continue
        else:
            continue
        planted[k].append(i)
    return d, planted


def count_ties(d, c=0.2, cv=0.2):
    """What the fp32 reference ops see: the number of positions with each tie / bound."""
    lp, v, olp, ov, adv, ret = (d[k].float() for k in ("lp", "v", "olp", "ov", "adv", "ret"))
    ratio = torch.exp(lp - olp)
    vclip = torch.clamp(v, ov - cv, ov + cv)
    vl1, vl2 = (v - ret) ** 2, (vclip - ret) ** 2
    lo, hi = float(np.float32(1.0) - np.float32(c)), float(np.float32(1.0) + np.float32(c))
    assert float(torch.clamp(torch.tensor(0.0), 1.0 - c, 1.0 + c)) == lo  # torch's bounds are these
    assert float(torch.clamp(torch.tensor(9.0), 1.0 - c, 1.0 + c)) == hi
    return {"v_lo": int((v == ov - cv).sum()), "v_hi": int((v == ov + cv).sum()),
            "ratio_lo": int((ratio == lo).sum()), "ratio_hi": int((ratio == hi).sum()),
            "adv0": int((adv == 0).sum()), "vl_tie_outside": int(((vl1 == vl2) & (v != vclip)).sum())}
