"""One decode step of a T5 decoder layer's attention over a device KV cache, fused.

  t5_relative_bias_table     HF's T5Attention.compute_bias for a decoder, as a [nH, max_len] fp32
                             table indexed by the distance t - j (built once per rollout)
  T5DecodeKVCache            k, v: [B, nH, max_len, d_kv] (HF's cache layout)
  t5_decode_self_attention   append k_new / v_new at column t, attend over columns 0..t with the
                             relative-position bias: one launch
  t5_decode_cross_attention  attend over the encoder's keys under its key mask: one launch
  T5DecodeClock              the decode position t as a device record: t5_decode_self_attention(t=clock)
                             reads it on the device, so a captured decode step replays per token
  t5_decode_embed            the decoder's input row of step t: the token drawn at step t - 1 (the
                             start token at 0) through the embedding table and, optionally, layer
                             0's first norm: one launch, t from a host int or the clock
  live=                      both attentions skip the rows whose entry of `live` is 0 (the
                             recorder's `unfinished`): zeros out, nothing read, the cache untouched
  t5_quantize_cross_kv       the encoder's keys / values to e4m3fn bytes with one power-of-two scale
                             per (row, head), once per rollout: one launch, a T5CrossKV8
  t5_decode_cross_attention_kv8   the cross-attention over those bytes: half the K / V traffic per
                             token, fp32 arithmetic; opt-in and lossy (3 mantissa bits)
  t5_decode_cross_attention_grouped   the cross-attention of a rollout that draws G samples per
                             prompt over ONE copy of each prompt's keys / values: K / V bytes per
                             token and K / V memory divided by G, every row bit-identical to
                             t5_decode_cross_attention on the repeat_interleave'd tensors

Per layer and generated token HF's eager T5Attention spends, between the projections and `o`, a
cache append, a [B, nH, 1, t] matmul, compute_bias (arange, bucket formula, embedding lookup,
permute), a mask add, a softmax and a second matmul.  trlx_t5_decode_attn (csrc/t5_decode_attn.hip)
does that in one launch with one workgroup per (batch row, head): fp32 dot products, fp32 bias add,
online fp32 softmax, fp32 P·V, one rounding.  T5 does not scale the scores by 1/sqrt(d_kv).
Forward only: generation runs under no_grad.

Kernel shapes: bfloat16 / float32 with d_kv 64 / 128.  For any other dtype or d_kv the two
functions evaluate the same step as torch expressions (`_torch_self_attention`,
`_torch_cross_attention`, HF's op order).
"""
import ctypes
import math

import torch

from . import _lib

__all__ = ["t5_relative_bias_table", "T5DecodeKVCache", "T5DecodeClock", "t5_decode_self_attention",
           "t5_decode_cross_attention", "t5_decode_embed", "T5CrossKV8", "t5_quantize_cross_kv",
           "t5_decode_cross_attention_kv8", "t5_decode_cross_attention_grouped"]

KERNEL_DTYPES = (torch.bfloat16, torch.float32)
KERNEL_D_KV = (64, 128)


def t5_relative_bias_table(weight, max_len, num_buckets=32, max_distance=128):
    """table[h, d] = weight[bucket(d), h] for the distances d = t - j in [0, max_len), fp32.

    weight: the decoder's relative_attention_bias.weight, [num_buckets, nH].  bucket is HF's
    unidirectional `_relative_position_bucket`, evaluated with the same float32 torch expression on
    the weight's device, so the buckets are HF's bit for bit: exact below num_buckets / 2, then
    logarithmic, saturating at max_distance.  The weights are frozen while generating: build it
    once per rollout."""
    if weight.dim() != 2 or weight.shape[0] != num_buckets:
        raise ValueError(f"weight must be [num_buckets = {num_buckets}, nH], got {tuple(weight.shape)}")
    if max_len < 1:
        raise ValueError(f"max_len = {max_len}")
    relative_position = torch.arange(max_len, dtype=torch.long, device=weight.device)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (
        torch.log(relative_position.float() / max_exact)
        / math.log(max_distance / max_exact)
        * (num_buckets - max_exact)
    ).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    buckets = torch.where(is_small, relative_position, if_large)
    return weight.detach().float()[buckets].t().contiguous()


class T5DecodeKVCache:
    """The self-attention cache of one decoder layer: k, v of [B, n_heads, max_len, d_kv], zeros."""

    def __init__(self, B, n_heads, d_kv, max_len, dtype, device):
        if min(B, n_heads, d_kv, max_len) < 1:
            raise ValueError(f"B, n_heads, d_kv, max_len = {B}, {n_heads}, {d_kv}, {max_len}")
        self.B, self.n_heads, self.d_kv, self.max_len = int(B), int(n_heads), int(d_kv), int(max_len)
        self.k = torch.zeros(B, n_heads, max_len, d_kv, dtype=dtype, device=device)
        self.v = torch.zeros(B, n_heads, max_len, d_kv, dtype=dtype, device=device)

    @property
    def dtype(self):
        return self.k.dtype

    @property
    def device(self):
        return self.k.device


class T5DecodeClock:
    """The decode position as a device record (trlx_decode_clock_init in trlx_t5_amd.h): int64 [8]
    = {t, T, cur_len0, overrun, 0, 0, 0, 0}.  t5_decode_self_attention(t=clock) and
    ppo_sample_step(recorder=PPORolloutRecorder(..., clock=clock)) read t from it on the device, so
    the launches of a decode step take the same arguments at every token and a step captured once
    (torch.cuda.graph) replays the whole rollout.

      T          the capacity: a step issued with t outside [0, T) does nothing
      cur_len0   HF's cur_len at t = 0 (1 for T5, the decoder start token)
      record     the int64 [8] tensor
      reset()    {0, T, cur_len0, 0, ...}: one launch, stream-ordered
      advance()  t < T ? t += 1 : overrun += 1: one launch, stream-ordered
      t, overrun host reads that synchronise: for after the rollout and for tests

    Nothing advances the clock implicitly: the caller's decode step ends with clock.advance(), one
    launch, after every call of the step that reads the clock.  On a CPU device the record exists
    for argument checks only and advance() raises."""

    def __init__(self, T, device, cur_len0=1):
        if isinstance(T, bool) or int(T) != T or int(T) < 1:
            raise ValueError(f"T5DecodeClock needs an integer capacity T >= 1, got {T!r}")
        if isinstance(cur_len0, bool) or int(cur_len0) != cur_len0 or int(cur_len0) < 0:
            raise ValueError(f"cur_len0 must be an integer >= 0, got {cur_len0!r}")
        self.T, self.cur_len0 = int(T), int(cur_len0)
        self.device = torch.device(device)
        self.record = torch.zeros(_lib.CLOCK_WORDS, dtype=torch.int64, device=self.device)
        self.reset()

    def reset(self):
        """t = 0, overrun = 0 (one launch on the current stream)."""
        if self.record.is_cuda:
            _lib.call("trlx_decode_clock_init", self.record.data_ptr(), self.T, self.cur_len0,
                      _lib.stream_of(self.record))
        else:
            self.record.copy_(torch.tensor([0, self.T, self.cur_len0, 0, 0, 0, 0, 0], dtype=torch.int64))

    def advance(self):
        """The end of a decode step: t += 1, or overrun += 1 once t has reached T (one launch)."""
        _lib.require_cuda(self.record)
        _lib.call("trlx_decode_clock_advance", self.record.data_ptr(), _lib.stream_of(self.record))

    @property
    def t(self):
        return int(self.record[_lib.CLOCK_T])

    @property
    def overrun(self):
        return int(self.record[_lib.CLOCK_OVERRUN])


def _rows(x, name, B, nH, d):
    """x as (tensor, row stride): [B, nH*d], [B, 1, nH*d], [B, nH, d] or [B, nH, 1, d] whose heads sit
    d apart with unit element stride are read in place; anything else is copied once."""
    inner = nH * d
    if x.dim() == 4 and tuple(x.shape) == (B, nH, 1, d):
        x = x[:, :, 0]
    elif x.dim() == 3 and tuple(x.shape) == (B, 1, inner):
        x = x[:, 0]
    if x.dim() == 3 and tuple(x.shape) == (B, nH, d):
        ok = x.stride(2) == 1 and (nH == 1 or x.stride(1) == d)
    elif x.dim() == 2 and tuple(x.shape) == (B, inner):
        ok = x.stride(1) == 1
    else:
        raise ValueError(f"{name} must be [B, nH*d_kv], [B, 1, nH*d_kv], [B, nH, d_kv] or [B, nH, 1, d_kv] with "
                         f"B, nH, d_kv = {B}, {nH}, {d}; got {tuple(x.shape)}")
    ld = x.stride(0)
    vec = 16 // x.element_size()
    if not ok or x.data_ptr() % 16 or (B > 1 and (ld < inner or ld % vec)):
        x = x.reshape(B, inner).contiguous()
        ld = inner
    return x, ld


def _check_q(q, B, nH, d, dtype, device):
    if not isinstance(q, torch.Tensor):
        raise TypeError(f"expected a tensor, got {type(q).__name__}")
    if q.dtype != dtype or q.device != device:
        raise ValueError(f"q / k_new / v_new must be {dtype} on {device} like the keys, got {q.dtype} on {q.device}")


def _kernel_takes(dtype, d):
    return dtype in KERNEL_DTYPES and d in KERNEL_D_KV


def _check_live(live, B, dtype, d, device):
    """The `live` argument of both attentions: a contiguous int64 [B] tensor on the keys' device."""
    if not isinstance(live, torch.Tensor):
        raise TypeError(f"live must be a tensor, got {type(live).__name__}")
    if live.dtype != torch.int64 or tuple(live.shape) != (B,) or live.device != device or not live.is_contiguous():
        raise ValueError(f"live must be a contiguous int64 [B] = [{B}] tensor on {device}, got {live.dtype} "
                         f"{tuple(live.shape)} on {live.device}")
    if not _kernel_takes(dtype, d):
        raise ValueError(f"live= needs the kernel ({KERNEL_DTYPES}, d_kv in {KERNEL_D_KV}); got {dtype}, d_kv {d}")


def _torch_self_attention(q, k_new, v_new, cache, t, bias_table):
    """The same step as torch expressions, HF's op order: append, matmul, bias add, fp32 softmax
    cast back, matmul."""
    B, nH, d = cache.B, cache.n_heads, cache.d_kv
    cache.k[:, :, t] = k_new.reshape(B, nH, d)
    cache.v[:, :, t] = v_new.reshape(B, nH, d)
    scores = torch.matmul(q.reshape(B, nH, 1, d), cache.k[:, :, :t + 1].transpose(2, 3))
    if bias_table is not None:
        dist = torch.arange(t, -1, -1, device=scores.device)
        scores = scores + bias_table[:, dist].to(scores.dtype)[None, :, None, :]
    w = torch.softmax(scores.float(), dim=-1).to(scores.dtype)
    return torch.matmul(w, cache.v[:, :, :t + 1]).reshape(B, nH * d)


def _torch_cross_attention(q, k_enc, v_enc, key_mask):
    B, nH, S, d = k_enc.shape
    scores = torch.matmul(q.reshape(B, nH, 1, d), k_enc.transpose(2, 3)).float()
    if key_mask is not None:
        scores = scores.masked_fill(key_mask[:, None, None, :] == 0, float("-inf"))
    w = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0).to(q.dtype)   # a fully masked row: zeros
    v = v_enc if key_mask is None else v_enc.masked_fill(key_mask[:, None, :, None] == 0, 0)
    return torch.matmul(w, v).reshape(B, nH * d)


def t5_decode_self_attention(q, k_new, v_new, cache, t, bias_table=None, live=None):
    """The self-attention of decode step t: k_new / v_new go to column t of `cache`, the query
    attends over columns 0..t with score_j = q·k_j + bias_table[h, t - j].  Returns [B, nH*d_kv].

    q, k_new, v_new: the projections of this token, [B, nH*d_kv], [B, 1, nH*d_kv], [B, nH, d_kv] or
    [B, nH, 1, d_kv] (HF's transposed view); row-strided views such as the three slices of a fused
    [B, 3*nH*d_kv] qkv projection are read in place.  t: a host int, 0 <= t < cache.max_len, or a
    T5DecodeClock on the cache's device with clock.T <= cache.max_len: the kernel then reads t from
    the clock (trlx_t5_decode_attn_dev), the call is the same launch at every token and can be
    captured; a live step is bit-identical to the call with that host t, a step with the clock at
    or past T (or below 0) returns zeros and leaves the cache alone.  The clock is not advanced
    here: the caller's step ends with clock.advance().  With a clock, a dtype or d_kv the kernel
    does not take raises ValueError (the torch fallback slices by a host t).
    bias_table: t5_relative_bias_table(...) for the layer that owns the bias, or None.
    live: None, or a contiguous int64 [B] tensor on the cache's device, 0 = skip the row
    (PPORolloutRecorder.unfinished as it is): a skipped row returns zeros, none of its q / k_new /
    v_new / cache is read and its column t of the cache stays unwritten; every other row has the
    bits of the call without `live` (trlx_t5_decode_attn_live, kernels of their own; live=None
    takes the entries it always took).  The skip is for recorders used with score_finished=False,
    the default: with score_finished=True the sampler would score the pad of a row whose attention
    was skipped.  Within one decode step every layer reads `live` before that step's sampling
    launch writes it: all of them are on one stream, in that order.
    Runs on the current stream, no host sync; only the output is allocated."""
    if not isinstance(cache, T5DecodeKVCache):
        raise TypeError("cache must be a T5DecodeKVCache")
    B, nH, d = cache.B, cache.n_heads, cache.d_kv
    clock = t if isinstance(t, T5DecodeClock) else None
    if clock is not None:
        if clock.T > cache.max_len:
            raise ValueError(f"the clock's capacity T = {clock.T} exceeds the cache's max_len = {cache.max_len}")
        if clock.device != cache.device:
            raise ValueError(f"the clock is on {clock.device}, the cache on {cache.device}")
        if not _kernel_takes(cache.dtype, d):
            raise ValueError(f"t=clock needs the kernel ({KERNEL_DTYPES}, d_kv in {KERNEL_D_KV}); the torch "
                             f"fallback for {cache.dtype}, d_kv {d} slices by a host t and cannot be captured")
        t = 0
    else:
        t = int(t)
        if not 0 <= t < cache.max_len:
            raise ValueError(f"t = {t} outside [0, max_len = {cache.max_len})")
    for x in (q, k_new, v_new):
        _check_q(x, B, nH, d, cache.dtype, cache.device)
    if bias_table is not None:
        if tuple(bias_table.shape) != (nH, cache.max_len) or bias_table.dtype != torch.float32 \
                or bias_table.device != cache.device or not bias_table.is_contiguous():
            raise ValueError(f"bias_table must be contiguous float32 [nH, max_len] = [{nH}, {cache.max_len}] on "
                             f"{cache.device}, got {bias_table.dtype} {tuple(bias_table.shape)}")
    if live is not None:
        _check_live(live, B, cache.dtype, d, cache.device)
    if not _kernel_takes(cache.dtype, d):
        return _torch_self_attention(q, k_new, v_new, cache, t, bias_table)
    _lib.require_cuda(cache.k, q, k_new, v_new)
    (q2, ldq), (k2, ldk), (v2, ldv) = (_rows(x, n, B, nH, d) for x, n in ((q, "q"), (k_new, "k_new"), (v_new, "v_new")))
    out = torch.empty(B, nH * d, dtype=cache.dtype, device=cache.device)
    args = _lib.T5DecodeAttnArgs(
        q=q2.data_ptr(), ldq=ldq, k_new=k2.data_ptr(), ldk=ldk, v_new=v2.data_ptr(), ldv=ldv,
        k=cache.k.data_ptr(), v=cache.v.data_ptr(), bias_by_distance=_lib.ptr(bias_table), key_mask=None,
        out=out.data_ptr(), B=B, n_heads=nH, d_kv=d, max_len=cache.max_len, t=t,
        dtype=_lib.dtype_code(cache.k), mode=_lib.T5_ATTN_SELF)
    if live is not None:
        _lib.call("trlx_t5_decode_attn_live", ctypes.byref(args), live.data_ptr(),
                  None if clock is None else clock.record.data_ptr(), _lib.stream_of(out))
    elif clock is not None:
        _lib.call("trlx_t5_decode_attn_dev", ctypes.byref(args), clock.record.data_ptr(), _lib.stream_of(out))
    else:
        _lib.call("trlx_t5_decode_attn", ctypes.byref(args), _lib.stream_of(out))
    return out


def t5_decode_cross_attention(q, k_enc, v_enc, key_mask=None, live=None):
    """The cross-attention of a decode step: score_j = q·k_enc_j over the keys with
    key_mask[b, j] != 0.  Returns [B, nH*d_kv].

    k_enc, v_enc: the encoder's projected keys / values, contiguous [B, nH, S, d_kv] (make HF's
    transposed view contiguous once per rollout).  key_mask: int64 [B, S], 0 = masked (the
    encoder's attention_mask; holes allowed), or None.  Masked keys are excluded from the softmax
    and not read; a row with every key masked returns zeros, where HF's additive finfo.min mask
    returns the plain average of the values.  q and live as in t5_decode_self_attention: a row
    with live[b] == 0 returns zeros and none of its q, keys, values or mask is read -- the S keys
    of a finished row are the larger part of what the skip saves.
    Runs on the current stream, no host sync; only the output is allocated."""
    if k_enc.dim() != 4 or k_enc.shape != v_enc.shape or k_enc.dtype != v_enc.dtype or k_enc.device != v_enc.device:
        raise ValueError("k_enc and v_enc must be [B, nH, S, d_kv] of one dtype on one device")
    B, nH, S, d = k_enc.shape
    if min(B, nH, S) < 1:
        raise ValueError(f"k_enc holds no key: shape {tuple(k_enc.shape)}")
    _check_q(q, B, nH, d, k_enc.dtype, k_enc.device)
    if key_mask is not None:
        if tuple(key_mask.shape) != (B, S) or key_mask.dtype != torch.int64 or key_mask.device != k_enc.device:
            raise ValueError(f"key_mask must be int64 [B, S] = [{B}, {S}] on {k_enc.device}, got {key_mask.dtype} "
                             f"{tuple(key_mask.shape)}")
    if live is not None:
        _check_live(live, B, k_enc.dtype, d, k_enc.device)
    if not _kernel_takes(k_enc.dtype, d):
        return _torch_cross_attention(q, k_enc, v_enc, key_mask)
    _lib.require_cuda(k_enc, q)
    if not (k_enc.is_contiguous() and v_enc.is_contiguous()):
        raise ValueError("k_enc and v_enc must be contiguous [B, nH, S, d_kv]: call .contiguous() once per rollout")
    if key_mask is not None and not key_mask.is_contiguous():
        key_mask = key_mask.contiguous()
    q2, ldq = _rows(q, "q", B, nH, d)
    out = torch.empty(B, nH * d, dtype=k_enc.dtype, device=k_enc.device)
    args = _lib.T5DecodeAttnArgs(
        q=q2.data_ptr(), ldq=ldq, k_new=None, ldk=0, v_new=None, ldv=0, k=k_enc.data_ptr(), v=v_enc.data_ptr(),
        bias_by_distance=None, key_mask=_lib.ptr(key_mask), out=out.data_ptr(), B=B, n_heads=nH, d_kv=d,
        max_len=S, t=0, dtype=_lib.dtype_code(k_enc), mode=_lib.T5_ATTN_CROSS)
    if live is not None:
        _lib.call("trlx_t5_decode_attn_live", ctypes.byref(args), live.data_ptr(), None, _lib.stream_of(out))
    else:
        _lib.call("trlx_t5_decode_attn", ctypes.byref(args), _lib.stream_of(out))
    return out


# ------------------------------------------------------------------ fp8 encoder keys and values
KV8_E_MIN, KV8_E_MAX = -100, 119    # the clamp of the scale's exponent (trlx_t5_cross_kv_quantize)
KV8_MAX = 448.0                     # the largest finite e4m3fn


class T5CrossKV8:
    """The encoder's keys and values of one decoder layer as e4m3fn bytes (t5_quantize_cross_kv).

      k8, v8             torch.float8_e4m3fn [B, nH, S, d_kv], contiguous
      k_scale, v_scale   float32 [B, nH], powers of two: key = k8 * k_scale[b, h]
      dequantize()       (K, V) in bfloat16, exact: byte * scale is representable in bf16, so
                         t5_decode_cross_attention on them sees the values the fp8 route computes on
    """

    def __init__(self, B, n_heads, S, d_kv, device):
        if min(B, n_heads, S) < 1 or d_kv not in KERNEL_D_KV:
            raise ValueError(f"B, n_heads, S = {B}, {n_heads}, {S} (>= 1), d_kv = {d_kv} (in {KERNEL_D_KV})")
        self.B, self.n_heads, self.S, self.d_kv = int(B), int(n_heads), int(S), int(d_kv)
        self.k8 = torch.zeros(B, n_heads, S, d_kv, dtype=torch.float8_e4m3fn, device=device)
        self.v8 = torch.zeros(B, n_heads, S, d_kv, dtype=torch.float8_e4m3fn, device=device)
        self.k_scale = torch.ones(B, n_heads, dtype=torch.float32, device=device)
        self.v_scale = torch.ones(B, n_heads, dtype=torch.float32, device=device)

    @property
    def device(self):
        return self.k8.device

    def dequantize(self):
        return tuple((x.float() * s[:, :, None, None]).to(torch.bfloat16)
                     for x, s in ((self.k8, self.k_scale), (self.v8, self.v_scale)))


def _torch_quantize_kv8(x, live, x8, scale):
    """One tensor of trlx_t5_cross_kv_quantize as torch expressions, bit for bit.  x: bf16
    [B, nH, S, d] (any strides), live: bool [B, S] or None."""
    B, nH, S, d = x.shape
    xf = x.float()
    if live is not None:
        xf = torch.where(live[:, None, :, None], xf, torch.zeros_like(xf))   # masked rows: not read, zero bytes
    amax = xf.abs().amax(dim=(2, 3))
    bad = ~torch.isfinite(amax)
    amax = torch.where(bad, torch.zeros_like(amax), amax)
    m, x2 = torch.frexp(amax)
    e = torch.where(m <= 0.875, x2 - 9, x2 - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(KV8_E_MIN, KV8_E_MAX)
    e = e.to(torch.int32)
    inv = ((127 - e) << 23).view(torch.float32)   # 2^-e, from its bits
    y =(xf * inv[:, :, None, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    nan_byte = torch.full_like(y, 0x7f)
    if live is not None:
        nan_byte = torch.where(live[:, None, :, None], nan_byte, torch.zeros_like(nan_byte))
    y = torch.where(bad[:, :, None, None], nan_byte, y)
    x8.view(torch.uint8).copy_(y)
    scale.copy_(torch.where(bad, torch.full_like(amax, float("nan")), ((127 + e) << 23).view(torch.float32)))


def _kv_strides(x, name, n_heads):
    """x as (tensor, (B, nH, S, d), (sb, sh, ss)): [B, nH, S, d] (HF's transposed view included) or
    the projection output [B, S, nH*d] with n_heads=; read in place when the last dimension has unit
    stride and the base and the other strides are whole 16-byte vectors, else copied once."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.bfloat16:
        raise ValueError(f"{name} must be a bfloat16 tensor")
    if x.dim() == 3:
        if n_heads is None or int(n_heads) < 1 or x.shape[2] % int(n_heads):
            raise ValueError(f"{name} is [B, S, nH*d_kv] = {tuple(x.shape)}: pass n_heads= (a divisor of the last dimension)")
        x = x.unflatten(2, (int(n_heads), x.shape[2] // int(n_heads))).permute(0, 2, 1, 3)   # a view
    elif x.dim() != 4:
        raise ValueError(f"{name} must be [B, nH, S, d_kv] or [B, S, nH*d_kv] with n_heads=, got {tuple(x.shape)}")
    B, nH, S, d = x.shape
    if n_heads is not None and int(n_heads) != nH:
        raise ValueError(f"{name} has {nH} heads, n_heads = {n_heads}")
    if min(B, nH, S) < 1 or d not in KERNEL_D_KV:
        raise ValueError(f"{name}: B, nH, S = {B}, {nH}, {S} (>= 1), d_kv = {d} (in {KERNEL_D_KV})")
    st = [x.stride(i) if x.shape[i] > 1 else 0 for i in range(3)]
    if x.stride(3) != 1 or x.data_ptr() % 16 or any(s < 0 or s % 8 for s in st) or \
            (nH > 1 and st[1] < d) or (S > 1 and st[2] < d):
        x = x.contiguous()
        st = [x.stride(i) if x.shape[i] > 1 else 0 for i in range(3)]
    return x, (B, nH, S, d), st


def t5_quantize_cross_kv(k_enc, v_enc, key_mask=None, out=None, n_heads=None):
    """The encoder's keys and values of one layer to e4m3fn, once per rollout: returns a T5CrossKV8.
    One launch for K and V (trlx_t5_cross_kv_quantize).

    k_enc, v_enc: bfloat16, [B, nH, S, d_kv] -- contiguous or HF's transposed view of the
    projection -- or the projection output [B, S, nH*d_kv] with n_heads=; d_kv 64 or 128.  Both are
    read in place: the .contiguous() that t5_decode_cross_attention asks for is not needed here.
    key_mask: int64 [B, S], 0 = masked, or None: a masked row is not read, is stored as zero bytes
    and does not enter the scale.  Per (b, h) and tensor: scale = 2^e with e the smallest integer
    such that max|x| * 2^-e <= 448 (0 for an all-zero block, clamped to [-100, 119]), byte =
    (x * 2^-e).to(torch.float8_e4m3fn), bit for bit.  A live Inf / NaN makes that block's scale NaN
    and its live bytes 0x7f: the attention gives NaN for that (b, h) only.
    out: a preallocated T5CrossKV8 of the same B, nH, S, d_kv on the same device, written in place.
    On a CPU device the same values come from torch expressions (`_torch_quantize_kv8`), bit for bit.
    Lossy against the bf16 keys: e4m3 keeps 3 mantissa bits.  Current stream, no host sync."""
    k, shape, k_st = _kv_strides(k_enc, "k_enc", n_heads)
    v, v_shape, v_st = _kv_strides(v_enc, "v_enc", n_heads)
    if shape != v_shape or k.device != v.device:
        raise ValueError(f"k_enc and v_enc differ: {shape} on {k.device}, {v_shape} on {v.device}")
    B, nH, S, d = shape
    if key_mask is not None:
        if not isinstance(key_mask, torch.Tensor) or tuple(key_mask.shape) != (B, S) or key_mask.dtype != torch.int64 \
                or key_mask.device != k.device:
            raise ValueError(f"key_mask must be int64 [B, S] = [{B}, {S}] on {k.device}")
        key_mask = key_mask.contiguous()
    if out is None:
        out = T5CrossKV8(B, nH, S, d, k.device)
    elif not isinstance(out, T5CrossKV8) or (out.B, out.n_heads, out.S, out.d_kv) != shape or out.device != k.device:
        raise ValueError(f"out must be a T5CrossKV8 of B, nH, S, d_kv = {shape} on {k.device}")
    if not k.is_cuda:
        live = None if key_mask is None else key_mask != 0
        _torch_quantize_kv8(k, live, out.k8, out.k_scale)
        _torch_quantize_kv8(v, live, out.v8, out.v_scale)
        return out
    args = _lib.T5CrossKvQuantArgs(
        k=k.data_ptr(), k_stride_b=k_st[0], k_stride_h=k_st[1], k_stride_s=k_st[2],
        v=v.data_ptr(), v_stride_b=v_st[0], v_stride_h=v_st[1], v_stride_s=v_st[2],
        key_mask=_lib.ptr(key_mask), k8=out.k8.data_ptr(), v8=out.v8.data_ptr(), k_scale=out.k_scale.data_ptr(),
        v_scale=out.v_scale.data_ptr(), B=B, n_heads=nH, S=S, d_kv=d)
    _lib.call("trlx_t5_cross_kv_quantize", ctypes.byref(args), _lib.stream_of(k))
    return out


def t5_decode_cross_attention_kv8(q, kv8, key_mask=None, live=None):
    """t5_decode_cross_attention over fp8 keys and values (trlx_t5_decode_attn_kv8): half the K / V
    bytes per token, the same fp32 arithmetic.  Returns bfloat16 [B, nH*d_kv].

    q: bfloat16, the shapes and strides of t5_decode_cross_attention.  kv8: a T5CrossKV8.
    key_mask, live: as in t5_decode_cross_attention.  score_j = (q · k8_j) * k_scale[b, h]; the
    output is (P · v8) * v_scale[b, h] / sum P, rounded once.  The result differs from the bf16
    route by the quantisation of K and V and by nothing else: t5_decode_cross_attention on
    kv8.dequantize() computes on the same values.  The launch takes the same arguments at every
    token and can be captured.  On a CPU device: the torch expressions on dequantize()."""
    if not isinstance(kv8, T5CrossKV8):
        raise TypeError("kv8 must be a T5CrossKV8")
    B, nH, S, d = kv8.B, kv8.n_heads, kv8.S, kv8.d_kv
    dev = kv8.device
    _check_q(q, B, nH, d, torch.bfloat16, dev)
    if key_mask is not None:
        if tuple(key_mask.shape) != (B, S) or key_mask.dtype != torch.int64 or key_mask.device != dev:
            raise ValueError(f"key_mask must be int64 [B, S] = [{B}, {S}] on {dev}, got {key_mask.dtype} "
                             f"{tuple(key_mask.shape)}")
    if live is not None:
        _check_live(live, B, torch.bfloat16, d, dev)
    if not kv8.k8.is_cuda:
        k, v = kv8.dequantize()
        out = _torch_cross_attention(q, k, v, key_mask)
        return out if live is None else torch.where((live != 0)[:, None], out, torch.zeros_like(out))
    for x in (kv8.k8, kv8.v8, kv8.k_scale, kv8.v_scale):
        if not x.is_contiguous():
            raise ValueError("kv8: k8, v8 and the scales must be contiguous")
    if key_mask is not None and not key_mask.is_contiguous():
        key_mask = key_mask.contiguous()
    q2, ldq = _rows(q, "q", B, nH, d)
    out = torch.empty(B, nH * d, dtype=torch.bfloat16, device=dev)
    args = _lib.T5DecodeAttnArgs(
        q=q2.data_ptr(), ldq=ldq, k_new=None, ldk=0, v_new=None, ldv=0, k=kv8.k8.data_ptr(), v=kv8.v8.data_ptr(),
        bias_by_distance=None, key_mask=_lib.ptr(key_mask), out=out.data_ptr(), B=B, n_heads=nH, d_kv=d,
        max_len=S, t=0, dtype=_lib.BF16, mode=_lib.T5_ATTN_CROSS)
    _lib.call("trlx_t5_decode_attn_kv8", ctypes.byref(args), kv8.k_scale.data_ptr(), kv8.v_scale.data_ptr(),
              _lib.ptr(live), _lib.stream_of(out))
    return out


# ------------------------------------------------------------------ keys shared by a prompt's samples
def _group_kv(x, name, n_heads):
    """x as a [P, nH, S, d] view: [P, nH, S, d] as it is, the projection output [P, S, nH*d] with
    n_heads= permuted (no copy)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(x).__name__}")
    if x.dim() == 3:
        if n_heads is None or int(n_heads) < 1 or x.shape[2] % int(n_heads):
            raise ValueError(f"{name} is [P, S, nH*d_kv] = {tuple(x.shape)}: pass n_heads= (a divisor of the last dimension)")
        x = x.unflatten(2, (int(n_heads), x.shape[2] // int(n_heads))).permute(0, 2, 1, 3)
    elif x.dim() != 4:
        raise ValueError(f"{name} must be [P, nH, S, d_kv] or [P, S, nH*d_kv] with n_heads=, got {tuple(x.shape)}")
    if n_heads is not None and int(n_heads) != x.shape[1]:
        raise ValueError(f"{name} has {x.shape[1]} heads, n_heads = {n_heads}")
    return x


def _group_strides(x):
    """(tensor, element strides over (p, h, s)) of a [P, nH, S, d] view for trlx_t5_decode_attn_group:
    read in place when d has unit stride and the base and the other strides are whole 16-byte
    vectors, else copied once.  The stride of a dimension of size 1 is passed as 0."""
    d, vec = x.shape[3], 16 // x.element_size()
    st = [x.stride(i) if x.shape[i] > 1 else 0 for i in range(3)]
    if x.stride(3) != 1 or x.data_ptr() % 16 or any(s < 0 or s % vec for s in st) or \
            (x.shape[1] > 1 and st[1] < d) or (x.shape[2] > 1 and st[2] < d):
        x = x.contiguous()
        st = [x.stride(i) if x.shape[i] > 1 else 0 for i in range(3)]
    return x, st


def t5_decode_cross_attention_grouped(q, k_enc, v_enc, key_mask=None, live=None, n_heads=None):
    """t5_decode_cross_attention for a rollout that draws G samples per prompt, over ONE copy of
    each prompt's keys and values (trlx_t5_decode_attn_group).  Returns [P*G, nH*d_kv].

    Row b = p * G + g of q, live and the result is sample g of prompt p: the order of
    repeat_interleave(G, dim=0), which is how HF expands num_return_sequences.  Every row has the
    bits of t5_decode_cross_attention(q, k_enc.repeat_interleave(G, 0).contiguous(), v_enc..., the
    mask repeated likewise): per query the kernel executes that kernel's floating-point operations
    in that kernel's order.  A key or value row is loaded once per (prompt, head, tile of queries)
    instead of once per sample, so K / V bytes per token and K / V memory drop by G.

    q: [P*G, nH*d_kv], [P*G, 1, nH*d_kv] or a row-strided view such as a slice of a fused projection,
    read in place as in t5_decode_cross_attention.  k_enc, v_enc: [P, nH, S, d_kv] (contiguous or
    HF's transposed view of the projection) or the projection output [P, S, nH*d_kv] with n_heads=;
    both are read in place through their strides, no .contiguous() is needed.  G = q.shape[0] //
    P; a batch that is not a whole multiple of P raises ValueError; G = 1 is the existing call.
    key_mask: int64 [P, S], per prompt, 0 = masked, or None; masked rows are not read; a fully
    masked prompt gives zeros in all its rows.  live: None or a contiguous int64 [P*G] tensor
    (PPORolloutRecorder.unfinished as it is): a dead row gets zeros and its q is not read, a prompt
    whose rows are all dead has none of its keys read, live rows keep the bits of the call without
    `live`.  The launch takes the same arguments at every token and can be captured.
    Tensors that are not on a ROCm device, another dtype or d_kv: whatever
    t5_decode_cross_attention does for the repeat_interleave'd operands.
    Runs on the current stream, no host sync; only the output is allocated."""
    k, v = _group_kv(k_enc, "k_enc", n_heads), _group_kv(v_enc, "v_enc", n_heads)
    if k.shape != v.shape or k.dtype != v.dtype or k.device != v.device:
        raise ValueError(f"k_enc and v_enc differ: {tuple(k.shape)} {k.dtype} on {k.device}, {tuple(v.shape)} "
                         f"{v.dtype} on {v.device}")
    P, nH, S, d = k.shape
    if min(P, nH, S) < 1:
        raise ValueError(f"k_enc holds no key: shape {tuple(k.shape)}")
    if not isinstance(q, torch.Tensor):
        raise TypeError(f"expected a tensor, got {type(q).__name__}")
    B = q.shape[0] if q.dim() else 0
    if B < P or B % P:
        raise ValueError(f"q has {B} rows, k_enc {P} prompts: the batch must be a whole multiple of the prompts "
                         f"(row p * G + g is sample g of prompt p)")
    G = B // P
    _check_q(q, B, nH, d, k.dtype, k.device)
    if key_mask is not None:
        if not isinstance(key_mask, torch.Tensor) or tuple(key_mask.shape) != (P, S) or key_mask.dtype != torch.int64 \
                or key_mask.device != k.device:
            raise ValueError(f"key_mask must be int64 [P, S] = [{P}, {S}] on {k.device}")
    if live is not None:
        _check_live(live, B, k.dtype, d, k.device)
    if not k.is_cuda or not _kernel_takes(k.dtype, d):
        return t5_decode_cross_attention(
            q, k.repeat_interleave(G, 0).contiguous(), v.repeat_interleave(G, 0).contiguous(),
            None if key_mask is None else key_mask.repeat_interleave(G, 0), live)
    _lib.require_cuda(k, q)
    if key_mask is not None and not key_mask.is_contiguous():
        key_mask = key_mask.contiguous()
    (k, k_st), (v, v_st) = _group_strides(k), _group_strides(v)
    q2, ldq = _rows(q, "q", B, nH, d)
    out = torch.empty(B, nH * d, dtype=k.dtype, device=k.device)
    args = _lib.T5DecodeAttnGroupArgs(
        q=q2.data_ptr(), ldq=ldq, k=k.data_ptr(), k_stride_p=k_st[0], k_stride_h=k_st[1], k_stride_s=k_st[2],
        v=v.data_ptr(), v_stride_p=v_st[0], v_stride_h=v_st[1], v_stride_s=v_st[2], key_mask=_lib.ptr(key_mask),
        live=_lib.ptr(live), out=out.data_ptr(), P=P, G=G, n_heads=nH, d_kv=d, S=S, dtype=_lib.dtype_code(k))
    _lib.call("trlx_t5_decode_attn_group", ctypes.byref(args), _lib.stream_of(out))
    return out


def t5_decode_cross_attention_group_tile(tile=0):
    """The largest query tile of t5_decode_cross_attention_grouped: 0 (the default, the measured
    choice), 1, 2, 4 or 8.  Process-wide; the result does not depend on it.  For the benchmark tool."""
    _lib.call("trlx_t5_decode_attn_group_tile", int(tile))


# ------------------------------------------------------------------ keys split across workgroups
SPLIT_MAX = 8            # the largest `splits` trlx_t5_decode_attn_split takes
_SPLIT_WORKSPACES = {}   # (device, bytes) -> uint8 tensor, allocated on first use and reused


def t5_decode_cross_attention_split_geometry(dtype, d_kv, S, splits):
    """trlx_t5_decode_attn_split_geometry as a dict (needs no device): NG groups of a workgroup, C
    keys a range (ceil(S / splits) rounded up to a multiple of NG), `ranges` = ceil(S / C) non-empty
    ranges, the query tile cap in force and max_splits."""
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}.get(dtype, -1)
    g = _lib.T5DecodeAttnSplitGeometry()
    _lib.call("trlx_t5_decode_attn_split_geometry", code, int(d_kv), int(S), int(splits), ctypes.byref(g))
    return {k: int(getattr(g, k)) for k, _ in g._fields_}


def t5_decode_cross_attention_split_plan(dtype, P, G, n_heads, d_kv, S):
    """The `splits` t5_decode_cross_attention_split takes by default for a shape
    (trlx_t5_decode_attn_split_plan): a pure function of the arguments, in 1 ... SPLIT_MAX, set from
    measurements; 1 for a dtype or d_kv the kernels do not take.  Needs no device."""
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}.get(dtype, -1)
    return int(_lib.query("trlx_t5_decode_attn_split_plan", code, int(P), int(G), int(n_heads), int(d_kv), int(S)))


def t5_decode_cross_attention_split_workspace_bytes(rows, n_heads, d_kv, splits):
    """trlx_t5_decode_attn_split_workspace_bytes: rows * n_heads * splits * (d_kv + 2) * 4."""
    return int(_lib.query("trlx_t5_decode_attn_split_workspace_bytes", int(rows), int(n_heads), int(d_kv), int(splits)))


def _split_workspace(device, nbytes):
    key = (device, nbytes)
    ws = _SPLIT_WORKSPACES.get(key)
    if ws is None:
        ws = _SPLIT_WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def t5_decode_cross_attention_split(q, k_enc, v_enc, key_mask=None, live=None, n_heads=None, groups=1, splits=None,
                                    workspace=None):
    """t5_decode_cross_attention_grouped with the S keys of every (row, head) cut into `splits`
    ranges, each walked by a workgroup of its own (trlx_t5_decode_attn_split): two launches, a partial
    pass that writes unnormalised fp32 states to a workspace and a merge.  For the shapes where the
    one-workgroup-per-(prompt, head, tile) grid leaves the chip under-filled.  Returns [P*G, nH*d_kv].

    q, k_enc, v_enc, key_mask, live, n_heads: as in t5_decode_cross_attention_grouped, with the same
    checks and the same in-place reading through strides.  groups: G, the samples a prompt; k_enc
    holds P = q.shape[0] // groups prompts and row p * G + g is sample g of prompt p.  groups=1 is
    the plain cross-attention.  splits: None = t5_decode_cross_attention_split_plan for the shape, or
    1 ... SPLIT_MAX; 1 is the grouped call, bit for bit.  For splits > 1 the result is
    bit-reproducible and depends on `splits` alone (not on P, the layout or the query tile), but is
    not the grouped call's bits: the merge order differs.
    workspace: None, or a contiguous tensor on the device of at least
    t5_decode_cross_attention_split_workspace_bytes(P*G, nH, d_kv, splits) bytes, 16-byte aligned.
    With None one is allocated on first use per (device, size) and reused by every later call, so
    nothing but the output is allocated per call and the call can be captured (call it once outside
    the capture first); calls that may run concurrently on different streams must pass workspaces
    of their own.  Tensors that are not on a ROCm device, another dtype or d_kv: what
    t5_decode_cross_attention_grouped does.  Runs on the current stream, no host sync."""
    k, v = _group_kv(k_enc, "k_enc", n_heads), _group_kv(v_enc, "v_enc", n_heads)
    if k.shape != v.shape or k.dtype != v.dtype or k.device != v.device:
        raise ValueError(f"k_enc and v_enc differ: {tuple(k.shape)} {k.dtype} on {k.device}, {tuple(v.shape)} "
                         f"{v.dtype} on {v.device}")
    P, nH, S, d = k.shape
    if min(P, nH, S) < 1:
        raise ValueError(f"k_enc holds no key: shape {tuple(k.shape)}")
    if not isinstance(q, torch.Tensor):
        raise TypeError(f"expected a tensor, got {type(q).__name__}")
    G = int(groups)
    B = q.shape[0] if q.dim() else 0
    if G < 1 or B != P * G:
        raise ValueError(f"q has {B} rows, k_enc {P} prompts, groups = {groups}: the batch must be prompts * groups "
                         f"(row p * G + g is sample g of prompt p)")
    if splits is not None and not 1 <= int(splits) <= SPLIT_MAX:
        raise ValueError(f"splits = {splits}: None (the plan) or 1 ... {SPLIT_MAX}")
    _check_q(q, B, nH, d, k.dtype, k.device)
    if key_mask is not None:
        if not isinstance(key_mask, torch.Tensor) or tuple(key_mask.shape) != (P, S) or key_mask.dtype != torch.int64 \
                or key_mask.device != k.device:
            raise ValueError(f"key_mask must be int64 [P, S] = [{P}, {S}] on {k.device}")
    if live is not None:
        _check_live(live, B, k.dtype, d, k.device)
    if not k.is_cuda or not _kernel_takes(k.dtype, d):
        return t5_decode_cross_attention_grouped(q, k_enc, v_enc, key_mask, live, n_heads)
    _lib.require_cuda(k, q)
    X = int(splits) if splits is not None else t5_decode_cross_attention_split_plan(k.dtype, P, G, nH, d, S)
    need = t5_decode_cross_attention_split_workspace_bytes(B, nH, d, X)
    if workspace is None:
        workspace = _split_workspace(k.device, need)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != k.device or not workspace.is_contiguous() \
            or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"workspace must be a contiguous tensor of at least {need} bytes on {k.device}")
    if key_mask is not None and not key_mask.is_contiguous():
        key_mask = key_mask.contiguous()
    (k, k_st), (v, v_st) = _group_strides(k), _group_strides(v)
    q2, ldq = _rows(q, "q", B, nH, d)
    out = torch.empty(B, nH * d, dtype=k.dtype, device=k.device)
    args = _lib.T5DecodeAttnGroupArgs(
        q=q2.data_ptr(), ldq=ldq, k=k.data_ptr(), k_stride_p=k_st[0], k_stride_h=k_st[1], k_stride_s=k_st[2],
        v=v.data_ptr(), v_stride_p=v_st[0], v_stride_h=v_st[1], v_stride_s=v_st[2], key_mask=_lib.ptr(key_mask),
        live=_lib.ptr(live), out=out.data_ptr(), P=P, G=G, n_heads=nH, d_kv=d, S=S, dtype=_lib.dtype_code(k))
    _lib.call("trlx_t5_decode_attn_split", ctypes.byref(args), X, workspace.data_ptr(),
              workspace.numel() * workspace.element_size(), _lib.stream_of(out))
    return out


EMBED_MAX_D = 8192   # the row tile of csrc/t5_rmsnorm.hip


def _torch_decode_embed(weight, tokens, t, start_token_id, norm_weight, eps):
    """The same step as torch expressions: the gather, F.embedding with zero rows for ids outside
    [0, V), HF's T5LayerNorm."""
    from .t5_norm import _torch_rmsnorm
    B, V = tokens.shape[0], weight.shape[0]
    tok = torch.full((B,), int(start_token_id), dtype=torch.int64, device=tokens.device) if t == 0 else tokens[:, t - 1]
    ok = (tok >= 0) & (tok < V)
    h = torch.nn.functional.embedding(torch.where(ok, tok, torch.zeros_like(tok)), weight)
    h = torch.where(ok[:, None], h, torch.zeros_like(h))
    return h, (None if norm_weight is None else _torch_rmsnorm(h, norm_weight, eps))


def t5_decode_embed(weight, tokens, t, start_token_id, norm_weight=None, eps=1e-6, out=None):
    """The decoder's input row of decode step t, one launch (trlx_t5_decode_embed): returns (h, y).

      tok = start_token_id at t == 0, else tokens[:, t - 1]      the token drawn at step t - 1
      h   = weight[tok]                                           bit for bit; T5 applies no scale
      y   = t5_rmsnorm(h, norm_weight, eps)                       bit for bit; None without norm_weight

    weight: [V, D] bfloat16 / float32 with unit element stride, rows any stride >= D apart (HF's
    shared.weight or a slice of it, read in place).  tokens: an int64 [B, T] tensor (row-strided
    views are read in place) or a PPORolloutRecorder, whose `.tokens` is used: a finished row holds
    pad there, which is what HF feeds.  A token outside [0, V) gives a zero row.  t: a host int in
    [0, T], or a T5DecodeClock: the kernel then reads t on the device, nothing is read on the host,
    the call is the same launch at every token and can be captured; the step is live iff
    0 <= t < clock.T and t - 1 < T, and a dead step writes zeros to h and y.  The clock is not
    advanced here.  norm_weight: [D] of weight's dtype, layer 0's first layer norm.  out=(h, y)
    (y None without norm_weight): preallocated [B, D] outputs with unit element stride, written in
    place, so that a captured step allocates nothing.  Forward only, current stream, no host sync.
    On a CPU device (host t only), or for another dtype or D > 8192, the same step runs as torch
    expressions."""
    if hasattr(tokens, "tokens") and not isinstance(tokens, torch.Tensor):
        tokens = tokens.tokens
    if not isinstance(weight, torch.Tensor) or not isinstance(tokens, torch.Tensor):
        raise TypeError("weight and tokens must be tensors (or tokens a PPORolloutRecorder)")
    if weight.dim() != 2 or min(weight.shape) < 1:
        raise ValueError(f"weight must be [V, D], got {tuple(weight.shape)}")
    if tokens.dim() != 2 or tokens.dtype != torch.int64 or min(tokens.shape) < 1 or tokens.device != weight.device:
        raise ValueError(f"tokens must be int64 [B, T] on {weight.device}, got {tokens.dtype} {tuple(tokens.shape)} "
                         f"on {tokens.device}")
    (V, D), (B, T) = weight.shape, tokens.shape
    if norm_weight is not None and (not isinstance(norm_weight, torch.Tensor) or tuple(norm_weight.shape) != (D,) or
                                    norm_weight.dtype != weight.dtype or norm_weight.device != weight.device):
        raise ValueError(f"norm_weight must be [D] = [{D}] {weight.dtype} on {weight.device}")
    clock = t if isinstance(t, T5DecodeClock) else None
    if clock is not None:
        if clock.device != weight.device:
            raise ValueError(f"the clock is on {clock.device}, weight on {weight.device}")
    else:
        t = int(t)
        if not 0 <= t <= T:
            raise ValueError(f"t = {t} outside [0, T = {T}]")
    kernel = weight.is_cuda and weight.dtype in KERNEL_DTYPES and D <= EMBED_MAX_D
    if out is not None:
        h, y = out
        for name, o, want in (("h", h, True), ("y", y, norm_weight is not None)):
            if (o is not None) != want:
                raise ValueError(f"out = (h, y): {name} must be {'a tensor' if want else 'None'} "
                                 f"{'with' if norm_weight is not None else 'without'} norm_weight")
            if o is not None and (tuple(o.shape) != (B, D) or o.dtype != weight.dtype or o.device != weight.device or
                                  o.stride(1) != 1):
                raise ValueError(f"out: {name} must be [B, D] = [{B}, {D}] {weight.dtype} on {weight.device} with unit "
                                 f"element stride")
    if not kernel:
        if clock is not None:
            raise ValueError(f"t=clock needs the kernel (a ROCm device, {KERNEL_DTYPES}, D <= {EMBED_MAX_D}); the torch "
                             f"fallback slices by a host t and cannot be captured")
        h2, y2 = _torch_decode_embed(weight, tokens, t, start_token_id, norm_weight, eps)
        if out is None:
            return h2, y2
        h.copy_(h2)
        if y is not None:
            y.copy_(y2)
        return h, y
    if weight.stride(1) != 1:
        raise ValueError("weight must have unit element stride (rows may be any stride >= D apart)")
    if tokens.stride(1) != 1 or (B > 1 and tokens.stride(0) < T):
        tokens = tokens.contiguous()
    if norm_weight is not None and not norm_weight.is_contiguous():
        norm_weight = norm_weight.contiguous()
    if out is None:
        h = torch.empty(B, D, dtype=weight.dtype, device=weight.device)
        y = torch.empty(B, D, dtype=weight.dtype, device=weight.device) if norm_weight is not None else None
    def ld(x, n):   # a single row has no stride to speak of
        return x.stride(0) if x.shape[0] > 1 else n

    args = _lib.T5DecodeEmbedArgs(
        weight=weight.data_ptr(), ld_w=ld(weight, D), tokens=tokens.data_ptr(), ld_tokens=ld(tokens, T),
        norm_w=_lib.ptr(norm_weight), h=h.data_ptr(), ld_h=ld(h, D), y=_lib.ptr(y), ld_y=D if y is None else ld(y, D),
        B=B, D=D, V=V, T=T, t=0 if clock is not None else t, start_token_id=int(start_token_id), eps=float(eps),
        dtype=_lib.dtype_code(weight))
    _lib.call("trlx_t5_decode_embed", ctypes.byref(args), None if clock is None else clock.record.data_ptr(),
              _lib.stream_of(h))
    return h, y
