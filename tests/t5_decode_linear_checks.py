"""Shared by the t5_decode_linear tests: the float64 oracle, the route the fused call replaces, the
shapes and the dispatch breaks of csrc/t5_decode_linear.hip.

The accuracy rule is the one of t5_attention_checks: with (b) the float64 oracle on the same bf16
inputs and (a) the existing route on the device (t5_rmsnorm / torch.matmul / the bf16 sum of
t5_add_rmsnorm / t5_ff_act_packed),

    max|kernel - (b)| <= 2 * max|(a) - (b)| + one bf16 ulp of max|(b)|
"""
import math

import torch

import trlx_t5_amd as P
from t5_attention_checks import bound  # noqa: F401  (the rule itself)

ACTS = ("relu", "gelu_new", "silu")
# (name, residual, act, gated): every epilogue
EPILOGUES = [("plain", False, None, False), ("residual", True, None, False)] + \
            [(a, False, a, False) for a in ACTS] + [("gated_" + a, False, a, True) for a in ACTS]
COMBOS = [(norm, epi) for norm in (False, True) for epi in EPILOGUES]


def combo_name(c):
    return ("norm+" if c[0] else "") + c[1][0]


# Where the kernel takes another path, by K.  Each is tested at K and at K + 32.
K_BREAKS = {
    128: "chunks 0-3 belong to wave 0: above, wave 1 has work (the waves' K split)",
    256: "above, wave 2 has work",
    384: "above, wave 3 has work",
    512: "above, wave 0 takes a second turn; the norm's sum of a lane spans a second unit (t5_rmsnorm's form break)",
    1024: "the norm's sum: one wave per row up to here, the whole workgroup per row above (form break)",
    2048: "the norm's sum of a thread spans a second unit above (form break)",
    4096: "a third and fourth unit above (form break)",
    8192: "t5_rmsnorm's limit: above, a norm weight is refused and only the other forms run",
}
# ... and by M (N 16, K 96): the row tiles per pass are 1, 4, 8, 16 (8 when gated); above 256 rows
# (128 gated) a second pass
M_BREAKS = (65, 129, 257)
MS, NS, KS = (1, 3, 16, 17, 33), (16, 48, 80), (32, 96, 256)
NORM_MAX_K = 8192
K_LARGEST = (3, 16, 16384)      # (M, N, K): the largest K taken


def shapes(norm):
    """(M, N, K) of the accuracy and determinism cases."""
    out = [(m, n, k) for m in MS for n in NS for k in KS]
    for b in K_BREAKS:
        for k in (b, b + 32):
            if not norm or k <= NORM_MAX_K:
                out.append((17, 16, k))
    out += [(m, 16, 96) for m in M_BREAKS]
    if not norm:
        out.append(K_LARGEST)
    return out


def max_err(x, ref):
    return float((x.detach().double() - ref.to(x.device)).abs().max())


def gelu_new64(u):
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))


def act64(u, act):
    return {"relu": torch.relu, "silu": lambda t: t * torch.sigmoid(t), "gelu_new": gelu_new64}[act](u)


def oracle(x, w, norm_w=None, eps=1e-6, residual=None, act=None, gated=False):
    """float64 on the given (bf16) inputs, nothing rounded in between."""
    x, w = x.double(), w.double()
    if norm_w is not None:
        x = norm_w.double() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    z = x @ w.t()
    if residual is not None:
        return z + residual.double()
    if act is None:
        return z
    if gated:
        f = z.shape[-1] // 2
        return act64(z[:, :f], act) * z[:, f:]
    return act64(z, act)


def unfused(x, w, norm_w=None, eps=1e-6, residual=None, act=None, gated=False):
    """The launches the fused call replaces, on the device."""
    y = x if norm_w is None else P.t5_rmsnorm(x, norm_w, eps)
    z = torch.matmul(y, w.t())
    if residual is not None:
        return P.t5_add_rmsnorm(z, residual, torch.ones(z.shape[-1], dtype=z.dtype, device=z.device))[0]
    if act is None:
        return z
    if gated:
        return P.t5_ff_act_packed(z, act)
    return P.t5_ff_act(z, None, act)


def inputs(M, N, K, gated, seed, device="cpu"):
    """x [M, K] with one row of magnitude 1e3 and one of 1e-3 (M >= 2), W ~ N(0, 1/K), a norm weight
    around 1 and a residual, all bf16."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[0] *= 1e3
    if M > 1:
        x[1] *= 1e-3
    w = torch.randn((2 if gated else 1) * N, K, generator=g) / math.sqrt(K)
    nw = 1.0 + 0.2 * torch.randn(K, generator=g)
    res = torch.randn(M, N, generator=g)
    return [t.to(torch.bfloat16).to(device) for t in (x, w, nw, res)]


def hf_block_state_dict(D, inner, F, gated, seed, prefix="decoder.block.0.", dtype=torch.bfloat16, device="cpu"):
    """A hand-built state dict with HF's names under one decoder block (plus the EncDecAttention k / v
    and the relative bias HF keeps there, which a decode step does not use)."""
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        return (torch.randn(o, i, generator=g) / math.sqrt(i)).to(dtype).to(device)

    sd = {}
    for n in "qkv":
        sd[f"layer.0.SelfAttention.{n}.weight"] = lin(inner, D)
    sd["layer.0.SelfAttention.o.weight"] = lin(D, inner)
    sd["layer.0.SelfAttention.relative_attention_bias.weight"] = torch.randn(32, 2, generator=g).to(dtype).to(device)
    for n in "qkv":
        sd[f"layer.1.EncDecAttention.{n}.weight"] = lin(inner, D)
    sd["layer.1.EncDecAttention.o.weight"] = lin(D, inner)
    if gated:
        sd["layer.2.DenseReluDense.wi_0.weight"], sd["layer.2.DenseReluDense.wi_1.weight"] = lin(F, D), lin(F, D)
    else:
        sd["layer.2.DenseReluDense.wi.weight"] = lin(F, D)
    sd["layer.2.DenseReluDense.wo.weight"] = lin(D, F)
    for i in range(3):
        sd[f"layer.{i}.layer_norm.weight"] = (1.0 + 0.2 * torch.randn(D, generator=g)).to(dtype).to(device)
    return {prefix + k: v for k, v in sd.items()}
