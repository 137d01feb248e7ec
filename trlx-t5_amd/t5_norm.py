"""T5's layer norm (HF T5LayerNorm: an RMSNorm, no mean subtraction, no bias, eps inside the root)
with the residual add of the sub-layer before it, one launch forward and at most two backward.

  t5_rmsnorm         y = weight * h * rsqrt(mean(h^2) + eps), differentiable in h and weight
  t5_add_rmsnorm     h = residual + x and y = norm(h) from one launch that reads x and residual once;
                     returns (h, y); differentiable in x, residual and weight
  T5LayerNorm        drop-in for HF's T5LayerNorm with HF's parameter name (`weight`) and attribute
                     (`variance_epsilon`); `add_forward(x, residual)` is the fused form

HF's eager T5LayerNorm is six elementwise / reduction launches over [N, d_model] in bf16, rounds
`h * rstd` and then `weight * (...)`, and its autograd keeps the fp32 upcast and the normalised
tensor; the add is one more launch.  trlx_t5_rmsnorm_fwd / _bwd (csrc/t5_rmsnorm.hip) keep a row in
registers from the sum of squares to the stores, compute in fp32 and round every output once; the
backward reads dy and h (and the gradient that reaches the residual stream from downstream) and
writes dh, and sums dw through per-workgroup fp32 partials and a fixed-order finish launch (no
atomics: bit-reproducible).  Saved for the backward: h, weight and rstd (fp32 [N]).

Kernel dtypes: bfloat16 and float32, with weight in the rows' dtype and D <= MAX_D.  Anything else
(float64, float16, a weight whose dtype differs from the rows' -- HF's fp32-weight case -- or a
wider row) evaluates HF's expressions as torch ops in HF's op order (`_torch_rmsnorm`); bfloat16 /
float32 tensors that are not on the device are refused, as `t5_ff_act` refuses them.
"""
import ctypes

import torch

from . import _lib
from .t5_ff import KERNEL_DTYPES, _ld, _rows

__all__ = ["t5_rmsnorm", "t5_add_rmsnorm", "T5LayerNorm", "geometry", "MAX_D", "VEC_BF16", "VEC_F32", "MAX_PARTIALS",
           "WAVE_ROW_MAX_D", "D_BREAKS"]

# the kernel's geometry (csrc/t5_rmsnorm.hip; trlx_t5_rmsnorm_geometry reports it)
VEC_BF16 = 8             # elements per 16-byte access
VEC_F32 = 4
MAX_D = 8192             # the widest row: 256 threads x 32 elements in registers
WAVE_ROW_MAX_D = 1024    # up to here one wave per row, 4 rows per workgroup pass; above, one row
MAX_PARTIALS = 1024      # G's cap
D_BREAKS = (512, 1024, 2048, 4096, 8192)   # the largest D of each kernel form


def geometry(N=0, D=0):
    """trlx_t5_rmsnorm_geometry for N rows of width D as a dict (needs no device)."""
    g = _lib.T5RmsNormGeometry()
    _lib.call("trlx_t5_rmsnorm_geometry", int(N), int(D), ctypes.byref(g))
    out = {name: getattr(g, name) for name, _ in g._fields_ if name not in ("d_breaks", "reserved", "n_breaks")}
    out["d_breaks"] = tuple(g.d_breaks[i] for i in range(g.n_breaks))
    return out


def _torch_rmsnorm(h, weight, eps):
    """HF's T5LayerNorm.forward as torch ops in its op order.  Differentiable.  The variance is taken
    in float32, or in float64 for float64 rows (HF's `.to(torch.float32)` would round those down)."""
    acc = torch.float64 if h.dtype == torch.float64 else torch.float32
    variance = h.to(acc).pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(variance + eps)
    if weight.dtype in (torch.float16, torch.bfloat16):
        h = h.to(weight.dtype)
    return weight * h


def _checked(who, h, weight, other=None):
    if not isinstance(h, torch.Tensor) or not isinstance(weight, torch.Tensor) or \
            (other is not None and not isinstance(other, torch.Tensor)):
        raise TypeError(f"{who}: the rows and weight must be tensors")
    if h.dim() < 1 or h.shape[-1] < 1:
        raise ValueError(f"{who}: rows must be [..., D] with D >= 1, got {tuple(h.shape)}")
    if weight.dim() != 1 or weight.shape[0] != h.shape[-1]:
        raise ValueError(f"{who}: weight must be [D] = [{h.shape[-1]}], got {tuple(weight.shape)}")
    if weight.device != h.device:
        raise ValueError(f"{who}: weight on {weight.device}, rows on {h.device}")
    if other is not None and (other.shape != h.shape or other.dtype != h.dtype or other.device != h.device):
        raise ValueError(f"{who}: x and residual must share shape, dtype and device, got {tuple(h.shape)} {h.dtype} "
                         f"{h.device} and {tuple(other.shape)} {other.dtype} {other.device}")
    return h.dtype in KERNEL_DTYPES and weight.dtype == h.dtype and h.shape[-1] <= MAX_D


def _launch(entry, first, N, D, eps, w=None, dw=None, rstd=None, ws=None, **rows):
    """One call on [N, D] rows (each of `rows` None or a 2-D view with unit element stride)."""
    kw = {}
    for name in ("x", "residual", "h", "y", "dy", "dh_in", "dh"):
        t = rows.get(name)
        kw[name] = _lib.ptr(t)
        kw[f"ld_{name}"] = D if t is None else _ld(t)
    args = _lib.T5RmsNormArgs(N=N, D=D, eps=eps, dtype=_lib.dtype_code(first), w=_lib.ptr(w), dw=_lib.ptr(dw),
                              rstd=_lib.ptr(rstd), ws=_lib.ptr(ws), ws_bytes=0 if ws is None else ws.numel() * 4, **kw)
    _lib.call(entry, ctypes.byref(args), _lib.stream_of(first))


def _keeps(*ts):
    """Whether a backward can follow: rstd is written and kept only then (inside a Function's forward
    grad mode is always off, so this is asked outside)."""
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _partials(N, D):
    rpb = 4 if D <= WAVE_ROW_MAX_D else 1
    return min((N + rpb - 1) // rpb, MAX_PARTIALS)


def _backward(ctx, g_h, g_y, want_dh, want_dw):
    """dh (the gradient of x and of residual, or of h) and dw from one backward."""
    h, weight, rstd = ctx.saved_tensors
    D = h.shape[-1]
    if g_y is None:                                            # y unused downstream: the norm passes nothing back
        return (g_h if want_dh else None), (torch.zeros_like(weight) if want_dw else None)
    h2 = _rows(h, D)
    N = h2.shape[0]
    dh = torch.empty(h.shape, dtype=h.dtype, device=h.device) if want_dh else None
    dw = torch.empty_like(weight) if want_dw else None
    if N == 0:
        return dh, (dw.zero_() if want_dw else None)
    ws = torch.empty(_partials(N, D), D, dtype=torch.float32, device=h.device) if want_dw else None
    _launch("trlx_t5_rmsnorm_bwd", h2, N, D, ctx.eps, w=weight, dw=dw, rstd=rstd, ws=ws, h=h2, dy=_rows(g_y, D),
            dh_in=_rows(g_h, D) if (g_h is not None and want_dh) else None, dh=None if dh is None else dh.view(-1, D))
    return dh, dw


class _T5RmsNormFn(torch.autograd.Function):
    """trlx_t5_rmsnorm_fwd / _bwd on h; saves h as given, weight and rstd."""

    @staticmethod
    def forward(ctx, h, weight, eps, keep):
        D = h.shape[-1]
        h2 = _rows(h.detach(), D)
        N = h2.shape[0]
        y = torch.empty(h.shape, dtype=h.dtype, device=h.device)
        rstd = torch.empty(N, dtype=torch.float32, device=h.device) if keep else None
        if N:
            _launch("trlx_t5_rmsnorm_fwd", h2, N, D, eps, w=weight.detach(), rstd=rstd, x=h2, y=y.view(-1, D))
        if keep:
            ctx.save_for_backward(h, weight, rstd)
        ctx.eps = eps
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        dh, dw = _backward(ctx, None, g_y, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dh, dw, None, None


class _T5AddRmsNormFn(torch.autograd.Function):
    """The add form: saves the h it returns, weight and rstd; one backward for dh (the gradient of
    both x and residual) and dw, taking the gradients of both outputs."""

    @staticmethod
    def forward(ctx, x, residual, weight, eps, keep):
        D = x.shape[-1]
        x2, r2 = _rows(x.detach(), D), _rows(residual.detach(), D)
        N = x2.shape[0]
        h = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        rstd = torch.empty(N, dtype=torch.float32, device=x.device) if keep else None
        if N:
            _launch("trlx_t5_rmsnorm_fwd", x2, N, D, eps, w=weight.detach(), rstd=rstd, x=x2, residual=r2,
                    h=h.view(-1, D), y=y.view(-1, D))
        if keep:
            ctx.save_for_backward(h, weight, rstd)
        ctx.eps = eps
        ctx.set_materialize_grads(False)
        return h, y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_h, g_y):
        want_dh = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if g_h is None and g_y is None:
            return None, None, None, None, None
        dh, dw = _backward(ctx, g_h, g_y, want_dh, ctx.needs_input_grad[2])
        return (dh if ctx.needs_input_grad[0] else None), (dh if ctx.needs_input_grad[1] else None), dw, None, None


def t5_rmsnorm(h, weight, eps=1e-6):
    """HF T5LayerNorm: weight * h * rsqrt(mean(h^2, -1) + eps), a new contiguous tensor shaped like h.

    h: [..., D]; weight: [D].  Rows that are D unit-stride elements one common stride apart
    (`h[:, -1, :]`, a [B, 1, D] decode slice, a padded buffer) are read in place; any other layout
    is copied once.  One launch; fp32 arithmetic, one rounding (HF's bf16 module rounds twice, so the
    bits differ from it and lie closer to the exact value).  Differentiable in h and weight: one row
    launch for dh, plus fp32 partials and a finish launch for dweight when weight needs a gradient
    (a frozen weight: no workspace, no second launch).  Saved: h as given, weight, rstd (fp32 [N]).
    No double backward.  Runs on the current stream with no host sync.  float64 / float16 rows, a
    weight of another dtype, or D > MAX_D evaluate HF's expressions as torch ops."""
    if not _checked("t5_rmsnorm", h, weight):
        return _torch_rmsnorm(h, weight, eps)
    _lib.require_cuda(h, weight)
    return _T5RmsNormFn.apply(h, weight, float(eps), _keeps(h, weight))


def t5_add_rmsnorm(x, residual, weight, eps=1e-6):
    """(h, y) with h = residual + x (bit for bit torch's sum) and y = t5_rmsnorm(h, weight, eps) (bit
    for bit), from one launch that reads x and residual once and writes h and y.

    The residual add of one T5 sub-layer folded into the next sub-layer's norm:
    `h, normed = t5_add_rmsnorm(attention_output, h, ln.weight)`.  Differentiable in x, residual and
    weight; the backward takes the gradients of both outputs (either may be absent) and runs once:
    dh = dnorm(dy) + dh_out is the gradient of x and of residual alike.  Everything else as t5_rmsnorm."""
    if not _checked("t5_add_rmsnorm", x, weight, residual):
        h = residual + x
        return h, _torch_rmsnorm(h, weight, eps)
    _lib.require_cuda(x, residual, weight)
    return _T5AddRmsNormFn.apply(x, residual, weight, float(eps), _keeps(x, residual, weight))


class T5LayerNorm(torch.nn.Module):
    """Drop-in for HF's T5LayerNorm: the same parameter (`weight`, ones) and attribute
    (`variance_epsilon`), so a state_dict loads with strict=True both ways.  forward(h) is
    `t5_rmsnorm`; add_forward(x, residual) is `t5_add_rmsnorm` and returns (h, y)."""

    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states):
        return t5_rmsnorm(hidden_states, self.weight, self.variance_epsilon)

    def add_forward(self, x, residual):
        return t5_add_rmsnorm(x, residual, self.weight, self.variance_epsilon)
