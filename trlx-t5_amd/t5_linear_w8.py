"""fp8 weights for the decode-step projections (opt-in, lossy; csrc/t5_decode_linear_w8.hip): the
weight-side counterpart of T5CrossKV8.

  t5_quantize_linear_weight   a bf16 nn.Linear.weight to e4m3fn bytes with one power-of-two scale per
                              output row, one launch: a T5LinearW8
  t5_decode_linear_w8         t5_decode_linear over those bytes: half the weight traffic per token, the
                              same prologue and epilogues, a streaming kernel of its own
  T5DecodeBlockWeights8       the six packed weights of a decoder block quantised; t5_decode_layer_fused
                              takes it in place of T5DecodeBlockWeights and runs the same 8 launches

At decode shapes a UL2-size projection is a read of its weight, so the bytes are the time.  The route
is exact against its own dequantize() (up to the order of one fp32 sum) and lossy against the bf16
weights: e4m3 keeps 3 mantissa bits.  The update's bf16 teacher-forced pass will not reproduce the
log-probs of a rollout drawn from fp8 weights exactly, and the weights must be quantised again after
every optimizer step (t5_quantize_linear_weight(w, out=...) writes in place).  No existing call
selects any of this.
"""
import ctypes

import torch

from . import _lib
from .t5_decode import _torch_quantize_kv8
from .t5_decode_linear import T5DecodeBlockWeights, _ld, _on_grid, _torch_decode_linear
from .t5_ff import ACTS, _act_code

__all__ = ["T5LinearW8", "t5_quantize_linear_weight", "t5_decode_linear_w8", "T5DecodeBlockWeights8", "linear_w8_geometry",
           "W8_COLS_PER_BLOCK", "W8_K_PER_CHUNK", "W8_MAX_K", "W8_NORM_MAX_K", "W8_WAVES"]

# the kernel's grid (trlx_t5_decode_linear_w8_geometry reports it)
W8_COLS_PER_BLOCK = 16     # N (F when gated) is a multiple of this
W8_K_PER_CHUNK = 64        # K is a multiple of this
W8_MAX_K = 16384
W8_NORM_MAX_K = 8192       # with norm_weight: t5_rmsnorm's limit
W8_WAVES = (4, 8, 16)      # waves of a workgroup, across which K is split


def linear_w8_geometry(N, K, gated=False):
    """trlx_t5_decode_linear_w8_geometry as a dict (needs no device): `waves` is the default the call
    takes for (N, K, gated), `turns` the 256-element turns of K that are dealt to the waves in turn."""
    g = _lib.T5DecodeLinearW8Geometry()
    _lib.call("trlx_t5_decode_linear_w8_geometry", int(N), int(K), int(bool(gated)), ctypes.byref(g))
    return {n: getattr(g, n) for n, _ in g._fields_}


class T5LinearW8:
    """A projection weight as e4m3fn bytes (t5_quantize_linear_weight).

      w8            torch.float8_e4m3fn [N, K], contiguous, nn.Linear.weight's [out, in] layout
      scale         float32 [N], powers of two: weight[n, k] = w8[n, k] * scale[n]
      dequantize()  bfloat16 [N, K], exact wherever byte * scale is a normal bf16 number: t5_decode_linear
                    on it sees the values the fp8 route computes on
    """

    def __init__(self, w8, scale):
        if not (isinstance(w8, torch.Tensor) and isinstance(scale, torch.Tensor)):
            raise TypeError("T5LinearW8: w8 and scale must be tensors")
        if w8.dtype != torch.float8_e4m3fn or w8.dim() != 2 or not w8.is_contiguous():
            raise ValueError(f"T5LinearW8: w8 must be a contiguous float8_e4m3fn [N, K], got {w8.dtype} {tuple(w8.shape)}")
        if scale.dtype != torch.float32 or tuple(scale.shape) != (w8.shape[0],) or scale.device != w8.device \
                or not scale.is_contiguous():
            raise ValueError(f"T5LinearW8: scale must be a contiguous float32 [{w8.shape[0]}] on {w8.device}, got "
                             f"{scale.dtype} {tuple(scale.shape)} on {scale.device}")
        self.w8, self.scale = w8, scale

    @property
    def shape(self):
        return self.w8.shape

    @property
    def device(self):
        return self.w8.device

    def dequantize(self):
        return (self.w8.float() * self.scale[:, None]).to(torch.bfloat16)


def t5_quantize_linear_weight(w, out=None):
    """A bf16 weight [N, K] to e4m3fn with one power-of-two scale per output row: returns a T5LinearW8.
    One launch (trlx_t5_linear_w8_quantize), one wave per row.

    w: bfloat16 [N, K] with unit element stride; the rows are read in place through their stride (a
    slice of a packed qkv or wi).  K a multiple of 8, at most 16384.  Per row: scale = 2^e with e the
    smallest integer such that max|w| * 2^-e <= 448 (0 for an all-zero row, clamped to [-100, 119]),
    byte = (w.float() * 2**-e).to(torch.float8_e4m3fn), bit for bit.  A row holding an Inf / NaN gets
    a NaN scale and 0x7f in every byte (t5_quantize_cross_kv's rule, per row): the projection gives NaN
    in that output column only.
    out: a T5LinearW8 of the same shape and device, written in place -- the form for quantising again
    after an optimizer step.  On a CPU device the same values come from torch expressions, bit for bit.
    Current stream, no host sync."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.bfloat16 or w.dim() != 2:
        raise ValueError("t5_quantize_linear_weight: w must be a bfloat16 [N, K] tensor")
    w = w.detach()
    N, K = w.shape
    if N < 1 or K < 8 or K % 8 or K > W8_MAX_K:
        raise ValueError(f"t5_quantize_linear_weight: w is [{N}, {K}]: N >= 1, K a multiple of 8 up to {W8_MAX_K}")
    if out is None:
        out = T5LinearW8(torch.empty(N, K, dtype=torch.float8_e4m3fn, device=w.device),
                         torch.empty(N, dtype=torch.float32, device=w.device))
    elif not isinstance(out, T5LinearW8) or tuple(out.shape) != (N, K) or out.device != w.device:
        raise ValueError(f"t5_quantize_linear_weight: out must be a T5LinearW8 of [{N}, {K}] on {w.device}")
    if not w.is_cuda:
        _torch_quantize_kv8(w[None, :, None, :], None, out.w8[None, :, None, :], out.scale[None])
        return out
    if not _on_grid(w):
        w = w.contiguous()
    if out.w8.data_ptr() % 16 or out.scale.data_ptr() % 16:
        raise ValueError("t5_quantize_linear_weight: out.w8 and out.scale must be 16-byte aligned")
    _lib.call("trlx_t5_linear_w8_quantize", w.data_ptr(), _ld(w), out.w8.data_ptr(), out.scale.data_ptr(), N, K,
              _lib.stream_of(w))
    return out


def t5_decode_linear_w8(x, w8, *, norm_weight=None, eps=1e-6, residual=None, act=None, gated=False, out=None, waves=None):
    """t5_decode_linear over fp8 weights: out = epilogue(prologue(x) @ (scale * w8).T) in one launch
    (trlx_t5_decode_linear_w8), bf16 MFMA with fp32 accumulation.

    x, norm_weight, eps, residual, act, gated, out: as t5_decode_linear takes them (bf16; x [B, K] or
    [B, 1, K] read in place; the normed rows carry t5_rmsnorm's bits; out may be the residual).  w8: a
    T5LinearW8 of [N, K] ([2F, K] when gated).  The bytes become bf16 in registers (exact) and the
    row's scale multiplies the fp32 sum once before the epilogue, so up to the order of one fp32 sum
    the result is t5_decode_linear's on w8.dequantize().
    waves: None, or 4 / 8 / 16: the waves of a workgroup, across which K is split in turns of 256.
    None takes the default for (N, K, gated) (linear_w8_geometry).  A row's bits depend on its x row,
    the weight row, K and waves -- not on B, N or the row's position; two calls give the same bits.
    Refused, with the reason: K not a multiple of 64 or above 16384, above 8192 with norm_weight, N
    not a multiple of 16, anything but bf16 x.  There is no rows-split, `live` or fp32 form.
    Forward only, current stream, no host sync, no allocation beyond `out`: the call can be captured.
    On a CPU device the same expression runs in torch on w8.dequantize()."""
    who = "t5_decode_linear_w8"
    if not isinstance(w8, T5LinearW8):
        raise TypeError(f"{who}: w8 must be a T5LinearW8 (t5_quantize_linear_weight)")
    ts = [t for t in (x, norm_weight, residual, out) if t is not None]
    if not all(isinstance(t, torch.Tensor) for t in ts):
        raise TypeError(f"{who}: x, norm_weight, residual and out must be tensors")
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise ValueError(f"{who} is forward only: an input requires grad (use torch.no_grad())")
    if act is not None:
        _act_code(act)
    if gated and act is None:
        raise ValueError(f"{who}: gated=True needs an act")
    if act is not None and residual is not None:
        raise ValueError(f"{who}: a residual and an act (one epilogue at most)")
    if waves is not None and waves not in W8_WAVES:
        raise ValueError(f"{who}: waves = {waves!r}: None or one of {W8_WAVES}")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"{who}: x must be bfloat16, got {x.dtype} (there is no fp32 form)")
    if x.dim() == 3 and x.shape[1] == 1:
        lead, x2 = (x.shape[0], 1), x[:, 0, :]
    elif x.dim() == 2:
        lead, x2 = (x.shape[0],), x
    else:
        raise ValueError(f"{who}: x must be [B, K] or [B, 1, K], got {tuple(x.shape)}")
    B, K = x2.shape
    rows = w8.shape[0]
    if w8.shape[1] != K or (gated and rows % 2):
        raise ValueError(f"{who}: w8 must be [{'2F' if gated else 'N'}, K = {K}], got {tuple(w8.shape)}")
    N = rows // 2 if gated else rows
    if B < 1:
        raise ValueError(f"{who}: x has no rows")
    if K % W8_K_PER_CHUNK or K > W8_MAX_K:
        raise ValueError(f"{who}: K = {K} must be a multiple of {W8_K_PER_CHUNK}, at most {W8_MAX_K}")
    if N % W8_COLS_PER_BLOCK or N < W8_COLS_PER_BLOCK:
        raise ValueError(f"{who}: N = {N} output columns must be a multiple of {W8_COLS_PER_BLOCK}")
    if norm_weight is not None and K > W8_NORM_MAX_K:
        raise ValueError(f"{who}: K = {K} with norm_weight is above {W8_NORM_MAX_K}, t5_rmsnorm's limit")
    if w8.device != x.device:
        raise ValueError(f"{who}: w8 is on {w8.device}, x on {x.device}")
    for name, t, shape in (("norm_weight", norm_weight, (K,)), ("residual", residual, (B, N)), ("out", out, (B, N))):
        if t is None:
            continue
        if t.dtype != x.dtype or t.device != x.device:
            raise ValueError(f"{who}: {name} must be {x.dtype} on {x.device}, got {t.dtype} on {t.device}")
        if tuple(t.shape if t.dim() != 3 else (t.shape[0], t.shape[2])) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)}, got {tuple(t.shape)}")
    r2 = residual if residual is None or residual.dim() == 2 else residual[:, 0, :]
    o2 = out if out is None or out.dim() == 2 else out[:, 0, :]
    if o2 is not None and o2.stride(1) != 1:
        raise ValueError(f"{who}: out must have unit element stride")

    if not x.is_cuda:
        got = _torch_decode_linear(x2, w8.dequantize(), norm_weight, eps, r2, act, gated)
        if out is None:
            return got.view(*lead, N)
        o2.copy_(got)
        return out

    if not _on_grid(x2):
        x2 = x2.contiguous()
    if norm_weight is not None and (not norm_weight.is_contiguous() or norm_weight.data_ptr() % 16):
        norm_weight = norm_weight.contiguous().clone()
    if r2 is not None and not _on_grid(r2):
        if o2 is not None and r2.data_ptr() == o2.data_ptr():
            raise ValueError(f"{who}: out is the residual, whose rows are off the kernel's grid (unit element stride, "
                             "16-byte aligned, row stride a multiple of 8)")
        r2 = r2.contiguous()
    if o2 is None:
        out = torch.empty(*lead, N, dtype=x.dtype, device=x.device)
        o2 = out.view(B, N)
    elif not _on_grid(o2):
        raise ValueError(f"{who}: out must be 16-byte aligned with a row stride that is a multiple of 8 elements")
    args = _lib.T5DecodeLinearW8Args(
        x=x2.data_ptr(), ld_x=_ld(x2), weight8=w8.w8.data_ptr(), ld_w=K, scale=w8.scale.data_ptr(),
        norm_weight=_lib.ptr(norm_weight), residual=_lib.ptr(r2), ld_residual=N if r2 is None else _ld(r2),
        out=o2.data_ptr(), ld_out=_ld(o2), M=B, K=K, N=N, eps=float(eps), dtype=_lib.BF16,
        act=_lib.T5_ACT_NONE if act is None else ACTS[act], gated=int(bool(gated)), waves=int(waves or 0), reserved=0)
    _lib.call("trlx_t5_decode_linear_w8", ctypes.byref(args), _lib.stream_of(x2))
    return out


class T5DecodeBlockWeights8:
    """T5DecodeBlockWeights with the six packed projection weights as T5LinearW8 (`qkv`, `o`, `cq`,
    `co`, `wi`, `wo`); the three norm weights `ln` stay bf16.  t5_decode_layer_fused takes it in place
    of the bf16 block.  Quantise again after every optimizer step: requantize(weights) writes the same
    buffers, six launches."""

    NAMES = ("qkv", "o", "cq", "co", "wi", "wo")

    def __init__(self, qkv, o, cq, co, wi, wo, ln, gated):
        self.qkv, self.o, self.cq, self.co, self.wi, self.wo, self.ln, self.gated = qkv, o, cq, co, wi, wo, tuple(ln), bool(gated)
        self.inner = qkv.shape[0] // 3
        self.d_model = qkv.shape[1]
        self.d_ff = wi.shape[0] // 2 if gated else wi.shape[0]

    @classmethod
    def from_weights(cls, w):
        if not isinstance(w, T5DecodeBlockWeights):
            raise TypeError("T5DecodeBlockWeights8.from_weights: a T5DecodeBlockWeights")
        return cls(*(t5_quantize_linear_weight(getattr(w, n)) for n in cls.NAMES), w.ln, w.gated)

    @classmethod
    def from_state_dict(cls, sd, prefix="", gated=True):
        return cls.from_weights(T5DecodeBlockWeights.from_state_dict(sd, prefix, gated))

    def requantize(self, w):
        """The bytes and scales of the bf16 block `w` into this block's buffers; returns self."""
        for n in self.NAMES:
            t5_quantize_linear_weight(getattr(w, n), out=getattr(self, n))
        self.ln = tuple(w.ln)
        return self

    def dequantize(self):
        """A T5DecodeBlockWeights of the dequantised weights: the bf16 block this one computes on."""
        return T5DecodeBlockWeights(*(getattr(self, n).dequantize() for n in self.NAMES), self.ln, self.gated)
