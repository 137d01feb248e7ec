"""T5's feed-forward block (HF T5LayerFF's DenseReluDense) with what sits between its projections
in one launch, forward and backward.

  t5_ff_act          act(u) * v (T5DenseGatedActDense: u = wi_0(x), v = wi_1(x)) or act(u) alone
                     (T5DenseActDense), differentiable
  t5_ff_act_packed   the same on one packed [..., 2F] projection output, u = uv[..., :F], v = uv[..., F:];
                     the backward writes both halves of one [..., 2F] gradient
  T5FeedForward      drop-in for HF's T5DenseGatedActDense / T5DenseActDense with HF's parameter names

act: "relu" (t5-base), "gelu_new" (HF's `gated-gelu` of T5 v1.1 / flan: the tanh form, not the erf
GELU) or "silu" (UL2's `gated-silu`).  HF's eager NewGELUActivation is about nine elementwise
launches over [N, d_ff], each rounded to the input dtype, and its autograd keeps every intermediate
for the backward; trlx_t5_ff_act_fwd / _bwd (csrc/t5_ff_act.hip) read u and v once, evaluate in fp32,
round every output once, and the backward recomputes act(u) from the saved u and v alone.  The
projections stay F.linear (hipBLASLt).

Kernel dtypes: bfloat16 and float32.  Any other dtype evaluates the same result as torch
expressions in HF's op order (`_torch_ff_act`); bfloat16 / float32 tensors that are not on the
device are refused, as `t5_attention` refuses them.
"""
import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib

__all__ = ["t5_ff_act", "t5_ff_act_packed", "T5FeedForward", "ACTS", "VEC_BF16", "VEC_F32", "COLS_PER_BLOCK",
           "ROWS_PER_BLOCK"]

ACTS = {"relu": _lib.T5_ACT_RELU, "gelu_new": _lib.T5_ACT_GELU_NEW, "silu": _lib.T5_ACT_SILU}
KERNEL_DTYPES = (torch.bfloat16, torch.float32)
# the kernel's geometry (csrc/t5_ff_act.hip; trlx_t5_ff_act_geometry reports it)
VEC_BF16 = 8            # elements per 16-byte access
VEC_F32 = 4
COLS_PER_BLOCK = 512    # columns per workgroup
ROWS_PER_BLOCK = 16     # rows per workgroup


def _act_code(act):
    if act not in ACTS:
        raise ValueError(f"act must be one of {sorted(ACTS)}, got {act!r} (HF's `gated-gelu` is 'gelu_new'; the erf "
                         f"GELU is not built)")
    return ACTS[act]


def _torch_ff_act(u, v, act):
    """The same result as torch expressions in HF's op order (NewGELUActivation / F.silu / relu,
    then the multiply).  Differentiable."""
    if act == "gelu_new":
        a = 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * torch.pow(u, 3.0))))
    elif act == "silu":
        a = F.silu(u)
    else:
        a = F.relu(u)
    return a if v is None else a * v


def _checked(u, v, act):
    code = _act_code(act)
    if not isinstance(u, torch.Tensor) or (v is not None and not isinstance(v, torch.Tensor)):
        raise TypeError("t5_ff_act: u and v must be tensors")
    if u.dim() < 1 or u.shape[-1] < 1:
        raise ValueError(f"t5_ff_act: u must be [..., F] with F >= 1, got {tuple(u.shape)}")
    if v is not None and (v.shape != u.shape or v.dtype != u.dtype or v.device != u.device):
        raise ValueError(f"t5_ff_act: u and v must share shape, dtype and device, got {tuple(u.shape)} {u.dtype} "
                         f"{u.device} and {tuple(v.shape)} {v.dtype} {v.device}")
    return code


def _rows(x, width):
    """x [..., width] as the [N, width] rows the kernel reads in place (unit element stride, one
    row stride >= width), else one contiguous copy."""
    try:
        x2 = x.view(-1, width)
    except RuntimeError:
        return x.reshape(-1, width).contiguous()
    ok = (width == 1 or x2.stride(1) == 1) and (x2.shape[0] <= 1 or x2.stride(0) >= width)
    return x2 if ok else x2.contiguous()


def _ld(x2):
    return x2.stride(0) if x2.shape[0] > 1 else x2.shape[1]


def _launch(entry, code, N, width, u=None, v=None, out=None, dy=None, du=None, dv=None):
    """One launch on [N, width] rows (each tensor None or a 2-D view with unit element stride)."""
    if N == 0:
        return
    first = u
    kw = {}
    for name, t in (("u", u), ("v", v), ("out", out), ("dy", dy), ("du", du), ("dv", dv)):
        kw[name] = _lib.ptr(t)
        kw[f"ld_{name}"] = width if t is None else _ld(t)
    args = _lib.T5FfActArgs(N=N, F=width, dtype=_lib.dtype_code(first), act=code, **kw)
    _lib.call(entry, ctypes.byref(args), _lib.stream_of(first))


class _T5FfActFn(torch.autograd.Function):
    """trlx_t5_ff_act_fwd / _bwd on separate u and v; saves u and v as given, nothing else."""

    @staticmethod
    def forward(ctx, u, v, code):
        width = u.shape[-1]
        u2 = _rows(u.detach(), width)
        v2 = None if v is None else _rows(v.detach(), width)
        out = torch.empty(u.shape, dtype=u.dtype, device=u.device)
        _launch("trlx_t5_ff_act_fwd", code, u2.shape[0], width, u=u2, v=v2, out=out.view(-1, width))
        ctx.save_for_backward(u, v)
        ctx.code = code
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        u, v = ctx.saved_tensors
        width = u.shape[-1]
        want_du = ctx.needs_input_grad[0]
        want_dv = v is not None and ctx.needs_input_grad[1]
        if not (want_du or want_dv):
            return None, None, None
        u2 = _rows(u, width)
        v2 = None if v is None else _rows(v, width)
        du = torch.empty(u.shape, dtype=u.dtype, device=u.device) if want_du else None
        dv = torch.empty(u.shape, dtype=u.dtype, device=u.device) if want_dv else None
        _launch("trlx_t5_ff_act_bwd", ctx.code, u2.shape[0], width, u=u2, v=v2, dy=_rows(dy, width),
                du=None if du is None else du.view(-1, width), dv=None if dv is None else dv.view(-1, width))
        return du, dv, None


class _T5FfActPackedFn(torch.autograd.Function):
    """The same on one packed [..., 2F] tensor; saves it as given, returns one [..., 2F] gradient."""

    @staticmethod
    def forward(ctx, uv, code):
        width = uv.shape[-1] // 2
        uv2 = _rows(uv.detach(), 2 * width)
        out = torch.empty(uv.shape[:-1] + (width,), dtype=uv.dtype, device=uv.device)
        _launch("trlx_t5_ff_act_fwd", code, uv2.shape[0], width, u=uv2[:, :width], v=uv2[:, width:],
                out=out.view(-1, width))
        ctx.save_for_backward(uv)
        ctx.code = code
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (uv,) = ctx.saved_tensors
        width = uv.shape[-1] // 2
        uv2 = _rows(uv, 2 * width)
        duv = torch.empty(uv.shape, dtype=uv.dtype, device=uv.device)
        d2 = duv.view(-1, 2 * width)
        _launch("trlx_t5_ff_act_bwd", ctx.code, uv2.shape[0], width, u=uv2[:, :width], v=uv2[:, width:],
                dy=_rows(dy, width), du=d2[:, :width], dv=d2[:, width:])
        return duv, None


def t5_ff_act(u, v=None, act="gelu_new"):
    """act(u) * v, or act(u) with v None: what HF's T5DenseGatedActDense / T5DenseActDense compute
    between their projections.  Returns a new contiguous tensor shaped like u.

    u, v: [..., F], one shape, dtype and device.  Rows that are `F` unit-stride elements one common
    stride apart (a slice of a packed projection output, a padded buffer) are read in place; any
    other layout is copied once.
    act: "relu", "gelu_new" (HF's `gated-gelu`) or "silu".
    Differentiable: the backward is one launch for du = dy v act'(u) and dv = dy act(u), recomputing
    act(u).  Saved for it: u and v as given — no activation, no product, no copy.  A gradient that is
    not needed (v.requires_grad False) is neither allocated nor computed.  No double backward.
    All arithmetic is fp32 and every output is rounded once, so bf16 results are closer to the exact
    value than HF's eager op sequence, which rounds every op.  Runs on the current stream with no
    host sync.  float64 / float16 operands evaluate the torch expressions of HF's modules."""
    code = _checked(u, v, act)
    if u.dtype not in KERNEL_DTYPES:
        return _torch_ff_act(u, v, act)
    _lib.require_cuda(u, v)
    return _T5FfActFn.apply(u, v, code)


def t5_ff_act_packed(uv, act="gelu_new"):
    """`t5_ff_act(uv[..., :F], uv[..., F:], act)` for a packed [..., 2F] projection output (one GEMM
    against the concatenated wi_0 / wi_1 weight): both halves are read in place, and the backward
    returns one [..., 2F] gradient whose halves the kernel wrote directly — autograd's slice
    backward would allocate and fill two zero tensors of the packed size instead.  Saved: uv as given."""
    code = _act_code(act)
    if not isinstance(uv, torch.Tensor):
        raise TypeError("t5_ff_act_packed: uv must be a tensor")
    if uv.dim() < 1 or uv.shape[-1] < 2 or uv.shape[-1] % 2:
        raise ValueError(f"t5_ff_act_packed: uv must be [..., 2F], got {tuple(uv.shape)}")
    if uv.dtype not in KERNEL_DTYPES:
        width = uv.shape[-1] // 2
        return _torch_ff_act(uv[..., :width], uv[..., width:], act)
    _lib.require_cuda(uv)
    return _T5FfActPackedFn.apply(uv, code)


class T5FeedForward(torch.nn.Module):
    """Drop-in for HF's T5DenseGatedActDense (config.is_gated_act) / T5DenseActDense with the
    activation and the gate in one launch (`t5_ff_act`).

    Parameter names are HF's — `wi_0.weight`, `wi_1.weight`, `wo.weight`, or `wi.weight`,
    `wo.weight` when not gated — so an HF module's state_dict loads with strict=True and the
    reverse.  The projections are F.linear.  No dropout is applied, whatever config.dropout_rate
    says: the reference trains with dropout off.  config.dense_act_fn must be one the kernel has
    ("relu", "gelu_new", "silu"); anything else raises here, not at the first forward."""

    def __init__(self, config):
        super().__init__()
        self.act = config.dense_act_fn
        _act_code(self.act)
        self.is_gated = bool(config.is_gated_act)
        if self.is_gated:
            self.wi_0 = torch.nn.Linear(config.d_model, config.d_ff, bias=False)
            self.wi_1 = torch.nn.Linear(config.d_model, config.d_ff, bias=False)
        else:
            self.wi = torch.nn.Linear(config.d_model, config.d_ff, bias=False)
        self.wo = torch.nn.Linear(config.d_ff, config.d_model, bias=False)

    def forward(self, hidden_states):
        if self.is_gated:
            h = t5_ff_act(self.wi_0(hidden_states), self.wi_1(hidden_states), self.act)
        else:
            h = t5_ff_act(self.wi(hidden_states), None, self.act)
        if h.dtype != self.wo.weight.dtype and self.wo.weight.dtype != torch.int8:   # HF keeps wo in fp32 for 8-bit loads
            h = h.to(self.wo.weight.dtype)
        return self.wo(h)
