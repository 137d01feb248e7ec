"""CPU restatements of one T5 decode-step attention (csrc/t5_decode_attn.hip) and the shared cases.

(b) oracle_*        float64, plain torch on the CPU, written from the definition: append, scores
                    (no 1/sqrt(d) scaling), the bias from HF's unidirectional buckets (evaluated in
                    Python floats per distance), the key mask, softmax, P·V.  A row whose keys are
                    all masked gives zeros (the kernel's documented deviation from HF's finfo.min).
(a) eager_*         torch's own route in the input dtype, HF's op order: matmul, bias / additive
                    mask add, fp32 softmax cast back, matmul.  Run on the device by the GPU test, it
                    supplies the error the kernel is measured against:
    bf16   max|kernel - (b)| <= max|(a) - (b)| + one bf16 ulp of max|(b)|   (the kernel rounds once
           where torch rounds scores, probabilities and the output)
    fp32   max|kernel - (b)| <= 4 * max|(a) - (b)|                          (summation order only)

Inputs: q and k are N(0, 1) * d_kv^-1/4, so that q·k ~ N(0, 1) (T5 initialises its q projection
for unscaled scores); v and the bias weights are N(0, 1).  Everything is generated in float32
from a seed, rounded to the case's dtype, and the oracle reads those rounded values.
"""
import math

import torch

B, NH, MAX_LEN = 3, 5, 160
NUM_BUCKETS, MAX_DISTANCE = 32, 128
D_KVS = (64, 128)
DTYPES = (torch.bfloat16, torch.float32)
# edges of one wave-wide load (8 keys at bf16 d_kv 64), of all waves' first round (32), of the bucket
# saturation (128) and the last column
SELF_T = (0, 7, 8, 9, 31, 32, 33, 127, 128, 129, 159)
CROSS_S = (1, 9, 33, 200)
MASKS = ("none", "right", "left", "holes")
LOOP_STEPS = 48


def dtype_name(dt):
    return {torch.bfloat16: "bf16", torch.float32: "fp32"}[dt]


# ------------------------------------------------------------------ bias
def bucket(distance, num_buckets=NUM_BUCKETS, max_distance=MAX_DISTANCE):
    """HF's unidirectional relative-position bucket of the distance t - j >= 0, in Python floats."""
    max_exact = num_buckets // 2
    if distance < max_exact:
        return distance
    large = max_exact + int(math.log(distance / max_exact) / math.log(max_distance / max_exact)
                            * (num_buckets - max_exact))
    return min(large, num_buckets - 1)


def oracle_bias_row(weight, t):
    """[nH, t + 1] float64: the bias of query t on keys 0..t from weight [num_buckets, nH]."""
    idx = torch.tensor([bucket(t - j, weight.shape[0]) for j in range(t + 1)])
    return weight.double()[idx].t()


# ------------------------------------------------------------------ (b) float64 oracle
def _attend(q, k, v, add=None, live=None):
    """q [B, nH, d], k / v [B, nH, n, d], add [.., nH, n] or None, live bool [B, n] or None -> [B, nH*d]."""
    s = torch.einsum("bhd,bhjd->bhj", q, k)
    if add is not None:
        s = s + add
    if live is not None:
        s = s.masked_fill(~live[:, None, :], float("-inf"))
        v = v.masked_fill(~live[:, None, :, None], 0.0)   # a masked value row may hold anything
    p = torch.softmax(s, dim=-1)
    if live is not None:
        p = torch.where(live.any(dim=1)[:, None, None], p, torch.zeros_like(p))
    return torch.einsum("bhj,bhjd->bhd", p, v).reshape(q.shape[0], -1)


def oracle_self_step(q, k_new, v_new, K, V, t, weight=None):
    """One self-attention step in float64.  q, k_new, v_new: [B, nH, d]; K, V: [B, nH, max_len, d]
    float64, column t written in place.  weight: [num_buckets, nH] or None."""
    K[:, :, t] = k_new.double()
    V[:, :, t] = v_new.double()
    add = None if weight is None else oracle_bias_row(weight, t)[None]
    return _attend(q.double(), K[:, :, :t + 1], V[:, :, :t + 1], add=add)


def oracle_cross(q, K, V, mask=None):
    """Cross-attention in float64: keys with mask[b, j] == 0 are excluded (their rows are not read:
    scores come from a copy with those rows zeroed)."""
    K, V = K.double(), V.double()
    live = None
    if mask is not None:
        live = mask != 0
        K = K.masked_fill(~live[:, None, :, None], 0.0)
    return _attend(q.double(), K, V, live=live)


# ------------------------------------------------------------------ (a) torch's eager route
def eager_self(q, K, V, t, bias_table=None):
    """HF's op order in the tensors' dtype on their device; K, V already hold column t."""
    Bq, nH, d = q.shape
    scores = torch.matmul(q.reshape(Bq, nH, 1, d), K[:, :, :t + 1].transpose(2, 3))
    if bias_table is not None:
        dist = torch.arange(t, -1, -1, device=q.device)
        scores = scores + bias_table[:, dist].to(scores.dtype)[None, :, None, :]
    w = torch.softmax(scores.float(), dim=-1).type_as(scores)
    return torch.matmul(w, V[:, :, :t + 1]).reshape(Bq, nH * d)


def eager_cross(q, K, V, mask=None):
    """K, V must hold finite values in the masked rows (HF's additive mask does not survive NaN)."""
    Bq, nH, d = q.shape
    scores = torch.matmul(q.reshape(Bq, nH, 1, d), K.transpose(2, 3))
    if mask is not None:
        add = torch.zeros(mask.shape, dtype=scores.dtype, device=q.device)
        add = add.masked_fill(mask == 0, torch.finfo(scores.dtype).min)
        scores = scores + add[:, None, None, :]
    w = torch.softmax(scores.float(), dim=-1).type_as(scores)
    return torch.matmul(w, V).reshape(Bq, nH * d)


# ------------------------------------------------------------------ cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def self_case(dtype, d_kv):
    """One token stream per (dtype, d_kv): Q, K, V [B, nH, MAX_LEN, d] in `dtype` (column t is step
    t's projections) and the bias weight [NUM_BUCKETS, nH] fp32."""
    g = _gen(1000 + d_kv + (7 if dtype == torch.float32 else 0))
    s = d_kv ** -0.25
    Q = (torch.randn(B, NH, MAX_LEN, d_kv, generator=g) * s).to(dtype)
    K = (torch.randn(B, NH, MAX_LEN, d_kv, generator=g) * s).to(dtype)
    V = torch.randn(B, NH, MAX_LEN, d_kv, generator=g).to(dtype)
    W = torch.randn(NUM_BUCKETS, NH, generator=g)
    return dict(Q=Q, K=K, V=V, W=W)


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


def cross_case(dtype, d_kv, S, kind):
    g = _gen(5000 + 13 * S + d_kv + (7 if dtype == torch.float32 else 0) + MASKS.index(kind))
    s = d_kv ** -0.25
    q = (torch.randn(B, NH, d_kv, generator=g) * s).to(dtype)
    K = (torch.randn(B, NH, S, d_kv, generator=g) * s).to(dtype)
    V = torch.randn(B, NH, S, d_kv, generator=g).to(dtype)
    return dict(q=q, K=K, V=V, mask=make_mask(kind, B, S, g))


def poison(x, mask):
    """x [B, nH, S, d] with NaN in the rows of the masked keys."""
    if mask is None:
        return x.clone()
    return x.masked_fill((mask == 0)[:, None, :, None], float("nan"))


# ------------------------------------------------------------------ the rule
def max_err(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max())


def bf16_ulp(magnitude):
    """One bf16 ulp at `magnitude` (8 significand bits)."""
    if magnitude <= 0:
        return 0.0
    return 2.0 ** (math.floor(math.log2(magnitude)) - 7)


def bound(dtype, e_torch, ref):
    if dtype == torch.bfloat16:
        return e_torch + bf16_ulp(float(ref.abs().max()))
    return 4.0 * e_torch
