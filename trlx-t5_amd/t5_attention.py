"""T5 attention over whole sequences, forward, in one launch: many queries against many keys
with the relative-position bias, the key mask and the causal rule inside the kernel.

  t5_relative_bias_offsets   HF's T5Attention.compute_bias(Tq, S) as a [nH, Tq + S - 1] fp32 table
                             indexed by key position minus query position (built once per shape)
  t5_relative_bias_buckets   the int64 [Tq + S - 1] bucket index by offset behind that table;
                             weight.float()[buckets].t().contiguous() is a differentiable table
  t5_attention               softmax(q·kᵀ + bias, over the live keys)·v -> [B, Tq, nH*d_kv]
  t5_attention_train         the same under autograd: trlx_t5_attention_fwd_lse forward, saving
                             q, k, v, out and the fp32 row statistics, and trlx_t5_attention_bwd
                             (csrc/t5_attention_bwd.hip) for dq, dk, dv and the bias table's gradient

The three many-query attentions of a T5 PPO rollout:
  encoder self-attention                 bias = bidirectional table, key_mask = attention_mask
  teacher-forced decoder self-attention  bias = unidirectional table, causal=True
  teacher-forced cross-attention         no bias, key_mask = the encoder's attention_mask, Tq != S

HF's eager T5Attention holds [B, nH, Tq, S] tensors for the scores, the bias, the mask sum and the
probabilities; trlx_t5_attention (csrc/t5_attention.hip) is a flash-attention forward on gfx950
MFMA that holds none of them: fp32 scores with the bias looked up per (i, j), an online fp32
softmax, P rounded to bf16 un-normalised as the P·V operand, O rescaled in fp32 and rounded once.
T5 does not scale the scores by 1/sqrt(d_kv).  `t5_attention` is forward only; the PPO update's
teacher-forced passes take `t5_attention_train`, whose backward recomputes the scores per tile and
saves nothing of size Tq x S either (no dropout: the reference trains with dropout off).

Kernel shapes: bfloat16 with d_kv 64 / 128.  For any other dtype or d_kv the call evaluates the
same result as torch expressions in HF's op order (`_torch_attention`).
"""
import ctypes
import math

import torch

from . import _lib

__all__ = ["t5_relative_bias_offsets", "t5_relative_bias_buckets", "t5_attention", "t5_attention_train", "Q_TILE",
           "KV_TILE", "BWD_DQ_Q_TILE", "BWD_DQ_KV_TILE", "BWD_DKV_K_TILE", "BWD_DKV_Q_TILE"]

# the kernel's tiles (kTaQTile, kTaKVTile in csrc/t5_attention.hip; trlx_t5_attention_tiles reports them)
Q_TILE = 128    # query rows per workgroup
KV_TILE = 64    # keys per LDS tile
# the backward's tiles (csrc/t5_attention_bwd.hip; trlx_t5_attention_bwd_tiles reports them)
BWD_DQ_Q_TILE = 128     # dq kernel: query rows per workgroup
BWD_DQ_KV_TILE = 64     # dq kernel: keys per LDS tile
BWD_DKV_K_TILE = 128    # dk / dv kernel: keys per workgroup
BWD_DKV_Q_TILE = 64     # dk / dv kernel: query rows per LDS tile
KERNEL_DTYPES = (torch.bfloat16,)
KERNEL_D_KV = (64, 128)


def t5_relative_bias_buckets(Tq, S, bidirectional, num_buckets=32, max_distance=128, device=None):
    """buckets[(j - i) + Tq - 1] = HF's `_relative_position_bucket` of key position j minus query
    position i (bidirectional for an encoder, unidirectional for a decoder): int64 [Tq + S - 1] on
    `device`, the float32 torch expression HF evaluates.  `weight.float()[buckets].t().contiguous()`
    is t5_relative_bias_offsets' table as a differentiable function of `weight`: build it once per
    step and hand the one tensor to every layer of the stack, so its gradient collects all of
    them, as HF's shared `position_bias` does."""
    if Tq < 1 or S < 1:
        raise ValueError(f"Tq, S = {Tq}, {S}")
    relative_position = torch.arange(-(Tq - 1), S, dtype=torch.long, device=device)   # j - i
    relative_buckets = torch.zeros_like(relative_position)
    nb = num_buckets
    if bidirectional:
        nb //= 2
        relative_buckets = relative_buckets + (relative_position > 0).to(torch.long) * nb
        relative_position = torch.abs(relative_position)
    else:
        relative_position = -torch.min(relative_position, torch.zeros_like(relative_position))
    max_exact = nb // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (
        torch.log(relative_position.float() / max_exact)
        / math.log(max_distance / max_exact)
        * (nb - max_exact)
    ).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, nb - 1))
    return relative_buckets + torch.where(is_small, relative_position, if_large)


def t5_relative_bias_offsets(weight, Tq, S, bidirectional, num_buckets=32, max_distance=128):
    """table[h, (j - i) + Tq - 1] = weight[bucket(j - i), h] for key j in [0, S) and query i in
    [0, Tq): fp32 [nH, Tq + S - 1].

    weight: relative_attention_bias.weight of the layer that owns the bias, [num_buckets, nH].
    bucket is HF's `_relative_position_bucket` (bidirectional for an encoder, unidirectional for a
    decoder), evaluated with the same float32 torch expression on the weight's device
    (t5_relative_bias_buckets), so table[h, j - i + Tq - 1] equals
    T5Attention.compute_bias(Tq, S)[0, h, i, j] bit for bit.  The weights are frozen during a
    rollout: build it once per (Tq, S).  Detached; for a table that carries gradients to `weight`
    index it with t5_relative_bias_buckets."""
    if weight.dim() != 2 or weight.shape[0] != num_buckets:
        raise ValueError(f"weight must be [num_buckets = {num_buckets}, nH], got {tuple(weight.shape)}")
    buckets = t5_relative_bias_buckets(Tq, S, bidirectional, num_buckets, max_distance, device=weight.device)
    return weight.detach().float()[buckets].t().contiguous()


def _as_bthd(x, name, layout, n_heads):
    """x as a [B, T, nH, d] view (no copy)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(x).__name__}")
    if x.dim() == 3:
        if n_heads is None or n_heads < 1 or x.shape[2] % n_heads:
            raise ValueError(f"{name} is [B, T, nH*d_kv] = {tuple(x.shape)}: pass n_heads= (a divisor of {x.shape[2]})")
        return x.unflatten(2, (n_heads, x.shape[2] // n_heads))
    if x.dim() != 4:
        raise ValueError(f"{name} must be [B, T, nH*d_kv], [B, T, nH, d_kv] or [B, nH, T, d_kv], got {tuple(x.shape)}")
    x = x if layout == "bthd" else x.transpose(1, 2)
    if n_heads is not None and x.shape[2] != n_heads:
        raise ValueError(f"{name} has {x.shape[2]} heads in layout {layout!r}, n_heads = {n_heads}")
    return x


def _in_place(x):
    """x [B, T, nH, d] if the kernel can read it where it is, else one contiguous copy."""
    d = x.shape[3]
    ok = x.stride(3) == 1 and x.data_ptr() % 16 == 0
    for dim in range(3):
        if x.shape[dim] > 1:
            s = x.stride(dim)
            ok = ok and s >= 0 and s % 8 == 0 and (dim == 0 or s >= d)
    return x if ok else x.contiguous()


def _torch_attention(q, k, v, bias, key_mask, causal, softmax_dtype=torch.float32):
    """The same result as torch expressions, HF's op order: matmul, the materialised bias, the
    excluded keys, fp32 softmax cast back, matmul.  q [B, Tq, nH, d], k / v [B, S, nH, d].
    Differentiable in q, k, v and bias; t5_attention_train keeps float64 operands' softmax in float64."""
    B, Tq, nH, d = q.shape
    S = k.shape[1]
    scores = torch.matmul(q.transpose(1, 2), k.permute(0, 2, 3, 1))                     # [B, nH, Tq, S]
    rel = torch.arange(S, device=q.device)[None, :] - torch.arange(Tq, device=q.device)[:, None]
    if bias is not None:
        scores = scores + bias[:, rel + (Tq - 1)].to(scores.dtype)[None]
    scores = scores.to(softmax_dtype)
    dead = torch.zeros(B, 1, Tq, S, dtype=torch.bool, device=q.device)
    if key_mask is not None:
        dead = dead | (key_mask == 0)[:, None, None, :]
    if causal:
        dead = dead | (rel > 0)[None, None]
    scores = scores.masked_fill(dead, float("-inf"))
    w = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0).to(q.dtype)             # no live key: zeros
    vv = v if key_mask is None else v.masked_fill((key_mask == 0)[:, :, None, None], 0)
    return torch.matmul(w, vv.transpose(1, 2)).transpose(1, 2).reshape(B, Tq, nH * d)


def _checked(q, k, v, bias, key_mask, causal, n_heads, layout, f64_bias=False):
    """The operands as [B, T, nH, d] views and their sizes, or the ValueError / TypeError both calls raise."""
    if layout not in ("bhtd", "bthd"):
        raise ValueError(f"layout must be 'bhtd' or 'bthd', got {layout!r}")
    if n_heads is None and bias is not None and isinstance(bias, torch.Tensor) and bias.dim() == 2:
        n_heads = int(bias.shape[0])
    q4, k4, v4 = (_as_bthd(x, n, layout, n_heads) for x, n in ((q, "q"), (k, "k"), (v, "v")))
    B, Tq, nH, d = q4.shape
    S = k4.shape[1]
    if min(B, Tq, nH, d, S) < 1:
        raise ValueError(f"empty operand: q {tuple(q.shape)}, k {tuple(k.shape)}")
    if tuple(k4.shape) != (B, S, nH, d) or v4.shape != k4.shape:
        raise ValueError(f"q, k, v disagree: [B, T, nH, d] = {tuple(q4.shape)}, {tuple(k4.shape)}, {tuple(v4.shape)}")
    if not (q4.dtype == k4.dtype == v4.dtype and q4.device == k4.device == v4.device):
        raise ValueError("q, k and v must share one dtype and one device")
    if causal and Tq != S:
        raise ValueError(f"causal needs Tq == S, got {Tq} and {S}")
    if bias is not None:
        f64 = f64_bias and isinstance(bias, torch.Tensor) and bias.dtype == q4.dtype == torch.float64
        if not isinstance(bias, torch.Tensor) or tuple(bias.shape) != (nH, Tq + S - 1) \
                or not (bias.dtype == torch.float32 or f64) or bias.device != q4.device:
            raise ValueError(f"bias must be float32 [nH, Tq + S - 1] = [{nH}, {Tq + S - 1}] on {q4.device} "
                             f"(t5_relative_bias_offsets), got {getattr(bias, 'dtype', None)} "
                             f"{tuple(getattr(bias, 'shape', ()))}")
    if key_mask is not None:
        if not isinstance(key_mask, torch.Tensor) or tuple(key_mask.shape) != (B, S) or key_mask.dtype != torch.int64 \
                or key_mask.device != q4.device:
            raise ValueError(f"key_mask must be int64 [B, S] = [{B}, {S}] on {q4.device}, got "
                             f"{getattr(key_mask, 'dtype', None)} {tuple(getattr(key_mask, 'shape', ()))}")
    return q4, k4, v4, (B, Tq, nH, d, S)


def t5_attention(q, k, v, *, bias=None, key_mask=None, causal=False, n_heads=None, layout="bhtd"):
    """T5's attention of Tq queries over S keys: score[i, j] = q_i·k_j + bias[h, (j - i) + Tq - 1]
    (unscaled), softmax over the keys that are not excluded, times v.  Returns [B, Tq, nH*d_kv],
    what the `o` projection takes.

    q: [B, Tq, ...], k, v: [B, S, ...], each in one of three forms, read in place:
      [B, T, nH*d_kv]   a projection's output or a slice of a fused [B, T, 3*nH*d_kv] projection;
                        needs n_heads=
      [B, nH, T, d_kv]  HF's `shape()` view or a contiguous cache (the layout the decode kernels'
                        k_enc / v_enc have); the default for 4-D operands, layout="bhtd"
      [B, T, nH, d_kv]  with layout="bthd"
    An operand is copied once only if it breaks the kernel's stride rules (unit element stride, a
    16-byte aligned base, every other stride a multiple of 8 elements).
    bias: t5_relative_bias_offsets(...), fp32 [nH, Tq + S - 1], or None.
    key_mask: int64 [B, S], 0 = excluded (the encoder's attention_mask; holes allowed), or None.
    Excluded keys' K and V rows are not read and may hold anything.  A query whose keys are all
    excluded returns zeros, where HF's additive finfo.min mask returns the plain average of v.
    causal: exclude the keys j > i; needs Tq == S.
    Runs on the current stream with no host sync; only the output is allocated.  Forward only:
    with an operand that requires grad under autograd it raises; where a backward is needed take
    the torch route, `t5_attention.torch_fallback(q, k, v, bias, key_mask, causal)` on [B, T, nH, d_kv]
    operands (the same expressions the other dtypes run), or HF's own T5Attention."""
    q4, k4, v4, (B, Tq, nH, d, S) = _checked(q, k, v, bias, key_mask, causal, n_heads, layout)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        raise RuntimeError("t5_attention is forward only: call it under torch.no_grad(), or take the torch fallback "
                           "t5_attention.torch_fallback(q, k, v, bias, key_mask, causal) on [B, T, nH, d_kv] operands "
                           "(or HF's T5Attention) where a backward is needed")
    if q4.dtype not in KERNEL_DTYPES or d not in KERNEL_D_KV:
        return _torch_attention(q4, k4, v4, bias, key_mask, bool(causal))
    _lib.require_cuda(q4)
    return _kernel_forward(_in_place(q4), _in_place(k4), _in_place(v4), bias, key_mask, causal, False)[0]


def _strides(field, prefix, x):
    """A [B, T, nH, d] tensor as the C structs take it: the pointer field and the three strides."""
    return {field: x.data_ptr(), f"{prefix}_stride_b": x.stride(0), f"{prefix}_stride_t": x.stride(1),
            f"{prefix}_stride_h": x.stride(2)}


def _kernel_forward(q4, k4, v4, bias, key_mask, causal, with_lse):
    """One launch on operands that meet the stride rules: (out [B, Tq, nH*d], lse fp32 [B, nH, Tq] or None)."""
    B, Tq, nH, d = q4.shape
    S = k4.shape[1]
    if bias is not None and not bias.is_contiguous():
        bias = bias.contiguous()
    if key_mask is not None and not key_mask.is_contiguous():
        key_mask = key_mask.contiguous()
    out = torch.empty(B, Tq, nH * d, dtype=q4.dtype, device=q4.device)
    args = _lib.T5AttentionArgs(
        **_strides("q", "q", q4), **_strides("k", "k", k4), **_strides("v", "v", v4),
        out=out.data_ptr(), o_stride_b=Tq * nH * d, o_stride_t=nH * d, o_stride_h=d,
        bias_by_offset=_lib.ptr(bias), key_mask=_lib.ptr(key_mask), B=B, n_heads=nH, d_kv=d, Tq=Tq, S=S,
        dtype=_lib.dtype_code(q4), causal=1 if causal else 0)
    if not with_lse:
        _lib.call("trlx_t5_attention", ctypes.byref(args), _lib.stream_of(out))
        return out, None
    lse = torch.empty(B, nH, Tq, dtype=torch.float32, device=q4.device)
    _lib.call("trlx_t5_attention_fwd_lse", ctypes.byref(args), lse.data_ptr(), _lib.stream_of(out))
    return out, lse


class _T5AttentionFn(torch.autograd.Function):
    """trlx_t5_attention_fwd_lse / trlx_t5_attention_bwd on [B, T, nH, d] bf16 operands."""

    @staticmethod
    def forward(ctx, q4, k4, v4, bias, key_mask, causal):
        q4, k4, v4 = _in_place(q4), _in_place(k4), _in_place(v4)
        if bias is not None:
            bias = bias.detach().contiguous()
        if key_mask is not None:
            key_mask = key_mask.contiguous()
        out, lse = _kernel_forward(q4.detach(), k4.detach(), v4.detach(), bias, key_mask, causal, True)
        ctx.save_for_backward(q4, k4, v4, out, lse, bias, key_mask)
        ctx.causal = bool(causal)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q4, k4, v4, out, lse, bias, key_mask = ctx.saved_tensors
        B, Tq, nH, d = q4.shape
        S = k4.shape[1]
        g4 = _in_place(dout.unflatten(2, (nH, d)))          # taken in place when it meets the stride rules
        o4 = out.unflatten(2, (nH, d))
        dq = torch.empty(B, Tq, nH, d, dtype=q4.dtype, device=q4.device)
        dk = torch.empty(B, S, nH, d, dtype=q4.dtype, device=q4.device)
        dv = torch.empty(B, S, nH, d, dtype=q4.dtype, device=q4.device)
        want_dbias = bias is not None and ctx.needs_input_grad[3]
        dbias = torch.empty(nH, Tq + S - 1, dtype=torch.float32, device=q4.device) if want_dbias else None
        ws_bytes = _lib.query("trlx_t5_attention_bwd_workspace_bytes", B, nH, Tq)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q4.device)
        args = _lib.T5AttentionBwdArgs(
            **_strides("q", "q", q4), **_strides("k", "k", k4), **_strides("v", "v", v4), **_strides("out", "o", o4),
            **_strides("dout", "do", g4), **_strides("dq", "dq", dq), **_strides("dk", "dk", dk),
            **_strides("dv", "dv", dv),
            lse=lse.data_ptr(), bias_by_offset=_lib.ptr(bias), key_mask=_lib.ptr(key_mask), dbias=_lib.ptr(dbias),
            workspace=ws.data_ptr(), workspace_bytes=ws_bytes, B=B, n_heads=nH, d_kv=d, Tq=Tq, S=S,
            dtype=_lib.dtype_code(q4), causal=1 if ctx.causal else 0)
        _lib.call("trlx_t5_attention_bwd", ctypes.byref(args), _lib.stream_of(dq))
        return dq, dk, dv, dbias, None, None


def t5_attention_train(q, k, v, *, bias=None, key_mask=None, causal=False, n_heads=None, layout="bhtd"):
    """`t5_attention` under autograd: the same operands, layouts and checks, the same result
    (bit for bit on the kernel's shapes), and gradients for q, k, v shaped like the tensors given and,
    when `bias.requires_grad`, the fp32 [nH, Tq + S - 1] gradient of the bias table.

    The teacher-forced passes of the PPO update (no dropout: the reference trains with it off).
    bias: to reach `relative_attention_bias.weight`, build the table as
    `weight.float()[t5_relative_bias_buckets(Tq, S, bidirectional, device=...)].t().contiguous()`
    once per step and pass the one tensor to every layer of the stack: its gradient then collects
    all of them, as HF's shared position_bias does.  A table that does not require grad (a frozen
    block) costs the backward nothing.
    Saved for the backward: q, k, v, out and the fp32 row statistics lse [B, nH, Tq] (and the bias and
    the mask) — nothing of size Tq x S; the backward recomputes the scores per tile
    (trlx_t5_attention_bwd: dq, dk, dv bit-reproducible, the bias gradient summed with fp32 atomics
    and not).  The incoming gradient is read in place when it meets the stride rules, else copied
    once.  No double backward.  Under torch.no_grad(), or with nothing that requires grad, this is
    `t5_attention`.  For other dtypes, other d_kv or CPU tensors the same torch expressions as
    `t5_attention`'s run under autograd; float64 operands stay in float64 throughout, softmax
    included, and may come with a float64 bias table."""
    q4, k4, v4, (B, Tq, nH, d, S) = _checked(q, k, v, bias, key_mask, causal, n_heads, layout, f64_bias=True)
    needs = torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (q, k, v, bias))
    if not needs:   # exactly t5_attention, for every dtype (a float64 table goes in as the float32 it takes)
        if bias is not None and bias.dtype != torch.float32:
            bias = bias.float()
        return t5_attention(q, k, v, bias=bias, key_mask=key_mask, causal=causal, n_heads=n_heads, layout=layout)
    if q4.dtype == torch.float64:   # no kernel either way: all of it in float64 (a float64 bias table is taken too)
        return _torch_attention(q4, k4, v4, bias, key_mask, bool(causal), softmax_dtype=torch.float64)
    if q4.dtype not in KERNEL_DTYPES or d not in KERNEL_D_KV or not q4.is_cuda:
        return _torch_attention(q4, k4, v4, bias, key_mask, bool(causal))
    return _T5AttentionFn.apply(q4, k4, v4, bias, key_mask, bool(causal))


# the package exports the function under the module's name: keep the tiles reachable either way
t5_attention.Q_TILE = Q_TILE
t5_attention.KV_TILE = KV_TILE
t5_attention.torch_fallback = _torch_attention
t5_attention_train.DQ_Q_TILE = BWD_DQ_Q_TILE
t5_attention_train.DQ_KV_TILE = BWD_DQ_KV_TILE
t5_attention_train.DKV_K_TILE = BWD_DKV_K_TILE
t5_attention_train.DKV_Q_TILE = BWD_DKV_Q_TILE
