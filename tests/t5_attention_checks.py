"""CPU restatements of T5's full-sequence attention (csrc/t5_attention.hip) and the shared cases.

(b) oracle          float64, plain torch on the CPU, written from the definition: unscaled scores,
                    the bias from HF's buckets evaluated in Python floats per (i, j), the key mask,
                    the causal rule, softmax, P·V.  A query whose keys are all excluded gives zeros
                    (the kernel's documented deviation from HF's finfo.min).
(a) eager           torch's own route in the input dtype, HF's op order: matmul, the materialised
                    [nH, Tq, S] bias plus the additive finfo.min mask, fp32 softmax cast back,
                    matmul.  Run on the device by the GPU test, it supplies the error the kernel is
                    measured against:
    max|kernel - (b)| <= 2 * max|(a) - (b)| + one bf16 ulp of max|(b)|
The factor 2: the kernel rounds P to bf16 as torch does, but un-normalised (before the division by
the row sum) and sums in another order, so its error is of torch's class, not below it.

Inputs: q and k are N(0, 1) * d_kv^-1/4 (q·k ~ N(0, 1): T5 initialises q for unscaled scores), v
and the bias weights are N(0, 1); generated in float32 from a seed and rounded to bf16, and the
oracle reads the rounded values.
"""
import math

import torch

B, NH = 2, 3
NUM_BUCKETS, MAX_DISTANCE = 32, 128
D_KVS = (64, 128)
MASKS = ("none", "right", "left", "holes")


def sizes(q_tile, kv_tile):
    """Self-attention lengths: one key, around one KV tile, past one Q tile, past two KV tiles, 200."""
    return sorted({1, kv_tile - 1, kv_tile, kv_tile + 1, q_tile + 1, 2 * kv_tile + 3, 200})


def cross_sizes(q_tile, kv_tile):
    return [(1, 200), (q_tile + 1, 1), (48, 2 * kv_tile + 3), (130, 33)]


# ------------------------------------------------------------------ bias
def bucket(rel, bidirectional, num_buckets=NUM_BUCKETS, max_distance=MAX_DISTANCE):
    """HF's relative-position bucket of rel = key position - query position, in Python floats."""
    base = 0
    if bidirectional:
        num_buckets //= 2
        if rel > 0:
            base = num_buckets
        rel = abs(rel)
    else:
        rel = max(-rel, 0)
    max_exact = num_buckets // 2
    if rel < max_exact:
        return base + rel
    large = max_exact + int(math.log(rel / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact))
    return base + min(large, num_buckets - 1)


def oracle_bias(weight, Tq, S, bidirectional, shift=0):
    """[nH, Tq, S] float64 from weight [num_buckets, nH]; shift moves every offset (a wrong index)."""
    idx = torch.tensor([[bucket(j - i + shift, bidirectional, weight.shape[0]) for j in range(S)] for i in range(Tq)])
    return weight.double()[idx].permute(2, 0, 1)


# ------------------------------------------------------------------ (b) float64 oracle
def oracle(q, k, v, weight=None, bidirectional=True, mask=None, causal=False, bias_shift=0, drop_key=None,
           causal_shift=0):
    """q [B, nH, Tq, d], k / v [B, nH, S, d] -> [B, Tq, nH*d] float64.  Excluded keys' rows are not
    read (they are zeroed in a copy first).  bias_shift, drop_key = (b, j) and causal_shift build
    the WRONG results the rule has to tell apart: the bias one offset off, one live key dropped,
    the causal boundary one off (causal_shift = -1 excludes the diagonal too)."""
    q, k, v = q.double(), k.double(), v.double()
    Bq, nH, Tq, d = q.shape
    S = k.shape[2]
    live = torch.ones(Bq, Tq, S, dtype=torch.bool)
    if mask is not None:
        live &= (mask != 0)[:, None, :]
    if drop_key is not None:
        live[drop_key[0], :, drop_key[1]] = False
    if causal:
        i, j = torch.arange(Tq)[:, None], torch.arange(S)[None, :]
        live &= (j <= i + causal_shift)[None]
    used = live.any(dim=1)                                       # [B, S]: read by some query
    k = k.masked_fill(~used[:, None, :, None], 0.0)
    v = v.masked_fill(~used[:, None, :, None], 0.0)
    s = torch.einsum("bhid,bhjd->bhij", q, k)
    if weight is not None:
        s = s + oracle_bias(weight, Tq, S, bidirectional, bias_shift)[None]
    s = s.masked_fill(~live[:, None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.where(live.any(dim=2)[:, None, :, None], p, torch.zeros_like(p))
    return torch.einsum("bhij,bhjd->bihd", p, v).reshape(Bq, Tq, nH * d)


# ------------------------------------------------------------------ (a) torch's eager route
def eager(q, k, v, bias=None, mask=None, causal=False):
    """HF's op order in the tensors' dtype on their device.  q [B, nH, Tq, d], k / v [B, nH, S, d];
    bias: the [nH, Tq + S - 1] offset table or None.  k, v must hold finite values in the masked
    rows (HF's additive mask does not survive NaN)."""
    Bq, nH, Tq, d = q.shape
    S = k.shape[2]
    scores = torch.matmul(q, k.transpose(3, 2))
    rel = torch.arange(S, device=q.device)[None, :] - torch.arange(Tq, device=q.device)[:, None]
    position_bias = torch.zeros(1, nH, Tq, S, dtype=scores.dtype, device=q.device)
    if bias is not None:
        position_bias = position_bias + bias[:, rel + (Tq - 1)].to(scores.dtype)[None]
    fmin = torch.finfo(scores.dtype).min
    if mask is not None:
        add = torch.zeros(mask.shape, dtype=scores.dtype, device=q.device).masked_fill(mask == 0, fmin)
        position_bias = position_bias + add[:, None, None, :]
    if causal:
        add = torch.zeros(Tq, S, dtype=scores.dtype, device=q.device).masked_fill(rel > 0, fmin)
        position_bias = position_bias + add[None, None]
    scores = scores + position_bias
    w = torch.softmax(scores.float(), dim=-1).type_as(scores)
    return torch.matmul(w, v).transpose(1, 2).reshape(Bq, Tq, nH * d)


# ------------------------------------------------------------------ cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_mask(kind, Bm, S, g):
    """int64 [B, S] or None; every row keeps at least one live key."""
    if kind == "none":
        return None
    m = torch.ones(Bm, S, dtype=torch.int64)
    for b in range(Bm):
        n = int(torch.randint(1, S + 1, (1,), generator=g))   # live keys
        if kind == "right":
            m[b, n:] = 0
        elif kind == "left":
            m[b, :S - n] = 0
        else:
            m[b] = (torch.rand(S, generator=g) < 0.5).long()
            m[b, int(torch.randint(0, S, (1,), generator=g))] = 1
    return m


def case(d_kv, Tq, S, kind="none", seed=0, Bc=B, nH=NH, dtype=torch.bfloat16):
    """q [B, nH, Tq, d], k / v [B, nH, S, d] in `dtype`, bias weight W [NUM_BUCKETS, nH] fp32 and the mask."""
    g = _gen(9000 + 131 * Tq + 17 * S + d_kv + MASKS.index(kind) + 100003 * seed)
    s = d_kv ** -0.25
    q = (torch.randn(Bc, nH, Tq, d_kv, generator=g) * s).to(dtype)
    k = (torch.randn(Bc, nH, S, d_kv, generator=g) * s).to(dtype)
    v = torch.randn(Bc, nH, S, d_kv, generator=g).to(dtype)
    W = torch.randn(NUM_BUCKETS, nH, generator=g)
    return dict(q=q, k=k, v=v, W=W, mask=make_mask(kind, Bc, S, g))


def poison(x, mask, value=float("nan")):
    """x [B, nH, S, d] with `value` in the rows of the masked keys."""
    if mask is None:
        return x.clone()
    return x.masked_fill((mask == 0)[:, None, :, None], value)


# ------------------------------------------------------------------ the rule
def max_err(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max())


def bf16_ulp(magnitude):
    """One bf16 ulp at `magnitude` (8 significand bits)."""
    if magnitude <= 0:
        return 0.0
    return 2.0 ** (math.floor(math.log2(magnitude)) - 7)


def bound(e_torch, ref):
    return 2.0 * e_torch + bf16_ulp(float(ref.abs().max()))
