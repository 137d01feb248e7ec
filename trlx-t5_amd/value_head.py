"""Drop-in for the PPO value head of trlx/model/nn/ppo_models.py on MI355X.

  make_head(n_embd, 1)   ppo_models.py:216-222: Linear(H, 2H).bfloat16(), ReLU, Linear(2H, 1).bfloat16()
  ValueHead              that nn.Sequential (the reference's modules and parameter names), its
                         forward fused; .values(h) is the squeezed hot-path form
  value_head             the function: values from hidden states, differentiable

The reference runs the head as three torch launches around an [N, 2H] bf16 activation
(ppo_models.py:618,:641).  trlx_value_head_fwd computes
  v_t = Σ_j relu(bf16(h_t·W1_j + b1_j)) · w2_j + b2
in one MFMA launch (a second small one when the 2H columns are split over workgroups) and never
writes the activation.  The backward recomputes it: trlx_value_head_bwd writes
dz = bf16(dv·w2·1[z > 0]), dw2, db1 and db2; dh = dz·W1 and dW1 = dzᵀ·h are plain GEMMs and go to
torch.matmul.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib

__all__ = ["ValueHead", "make_head", "value_head", "value_head_splits"]

H_MIN, H_MAX, H_STEP = 32, 8192, 32
_LD_MAX = 1 << 24


def _check(h, w1, b1, w2, b2, out_dtype):
    """Every argument check, before any library call.  Returns (lead shape, N, H)."""
    for name, t in (("h", h), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.bfloat16:
            raise TypeError(f"{name} must be bfloat16 (the reference's value head is bf16), got {t.dtype}")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    if h.dim() < 1:
        raise ValueError("h must be [..., H]")
    H = h.shape[-1]
    if H < H_MIN or H > H_MAX or H % H_STEP:
        raise ValueError(f"H = {H}: the fused value head takes {H_MIN} <= H <= {H_MAX}, H a multiple of {H_STEP}")
    if tuple(w1.shape) != (2 * H, H):
        raise ValueError(f"w1 must be [2H, H] = [{2 * H}, {H}] (nn.Linear layout), got {tuple(w1.shape)}")
    if tuple(b1.shape) != (2 * H,):
        raise ValueError(f"b1 must be [{2 * H}], got {tuple(b1.shape)}")
    if tuple(w2.shape) not in ((2 * H,), (1, 2 * H)):
        raise ValueError(f"w2 must be [{2 * H}] or [1, {2 * H}], got {tuple(w2.shape)}")
    if b2.numel() != 1:
        raise ValueError(f"b2 must hold one element, got {tuple(b2.shape)}")
    lead = tuple(h.shape[:-1])
    N = 1
    for d in lead:
        N *= d
    if N < 1:
        raise ValueError(f"h holds no token: shape {tuple(h.shape)}")
    _lib.require_cuda(h, w1, b1, w2, b2)
    if len({t.device for t in (h, w1, b1, w2, b2)}) != 1:
        raise ValueError("h, w1, b1, w2 and b2 must live on one device")
    return lead, N, H


def _rows(h, H):
    """h as [N, H] rows the kernel can read in place (unit column stride, one row stride that is a
    multiple of 8 elements, a 16-byte aligned base); anything else is copied."""
    h2 = h if h.dim() == 2 else h.reshape(-1, H)
    ld = h2.stride(0)
    if h2.stride(1) != 1 or h2.data_ptr() % 16 or (h2.shape[0] > 1 and (ld < H or ld % 8 or ld > _LD_MAX)):
        h2 = h2.contiguous()
    return h2


def _dense(t):
    if not t.is_contiguous():
        return t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def value_head_splits(N: int, H: int) -> int:
    """Column splits the forward uses for N tokens (a function of N, H and the device's compute
    units; `_lib.tuning(vhead_splits=S)` overrides it, capped at one split per 32 columns)."""
    return int(_lib.query("trlx_value_head_splits", int(N), int(H)))


def _forward(h, w1, b1, w2, b2, out_dtype, lead, N, H):
    h2 = _rows(h.detach(), H)
    w1c, b1c, w2c, b2c = (_dense(t.detach()) for t in (w1, b1, w2, b2))
    out = torch.empty(lead, dtype=out_dtype, device=h.device)
    ws = None
    if value_head_splits(N, H) > 1:
        ws = torch.empty(_lib.query("trlx_value_head_workspace_bytes", N, H), dtype=torch.uint8, device=h.device)
    _lib.call("trlx_value_head_fwd", h2.data_ptr(), h2.stride(0), w1c.data_ptr(), b1c.data_ptr(), w2c.data_ptr(),
              b2c.data_ptr(), N, H, out.data_ptr(), _lib.dtype_code(out), _lib.ptr(ws), _lib.stream_of(h))
    return out


class _ValueHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, out_dtype):
        lead, N, H = _check(h, w1, b1, w2, b2, out_dtype)
        out = _forward(h, w1, b1, w2, b2, out_dtype, lead, N, H)
        ctx.save_for_backward(h, w1, b1, w2)
        ctx.b2_shape = tuple(b2.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dv):
        h, w1, b1, w2 = ctx.saved_tensors
        H = h.shape[-1]
        N = h.numel() // H
        if dv.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"the gradient of the values must be float32 or bfloat16, got {dv.dtype}")
        dvc = dv.reshape(-1).contiguous()
        h2 = _rows(h, H)
        w1c, b1c, w2c = _dense(w1), _dense(b1), _dense(w2)
        dev = h.device
        dz = torch.empty((N, 2 * H), dtype=torch.bfloat16, device=dev)
        dw2 = torch.empty(2 * H, dtype=torch.bfloat16, device=dev)
        db1 = torch.empty(2 * H, dtype=torch.bfloat16, device=dev)
        db2 = torch.empty(1, dtype=torch.bfloat16, device=dev)
        ws = torch.empty(_lib.query("trlx_value_head_bwd_workspace_bytes", N, H), dtype=torch.uint8, device=dev)
        _lib.call("trlx_value_head_bwd", h2.data_ptr(), h2.stride(0), w1c.data_ptr(), b1c.data_ptr(),
                  w2c.data_ptr(), dvc.data_ptr(), _lib.dtype_code(dvc), N, H, dz.data_ptr(), dw2.data_ptr(),
                  db1.data_ptr(), db2.data_ptr(), _lib.BF16, ws.data_ptr(), _lib.stream_of(h))
        need = ctx.needs_input_grad
        # the two plain GEMMs of the head's backward go to the BLAS library
        dh = torch.matmul(dz, w1c).reshape(h.shape) if need[0] else None
        dw1 = torch.matmul(dz.t(), h2) if need[1] else None
        return (dh, dw1, db1 if need[2] else None, dw2.reshape(w2.shape) if need[3] else None,
                db2.reshape(ctx.b2_shape) if need[4] else None, None)


def value_head(h, w1, b1, w2, b2, out_dtype=torch.float32):
    """values = relu(bf16(h @ w1.T + b1)) @ w2 + b2 of shape h.shape[:-1], fused.

    h: bf16 [..., H] (a row-strided 2-D view such as h3[:, -1, :] is read in place); w1 [2H, H],
    b1 [2H], w2 [2H] or [1, 2H], b2 [1]: the bf16 parameters of make_head(H, 1).  32 <= H <= 8192,
    H a multiple of 32.  out_dtype float32 (default) or bfloat16: fp32 accumulation, rounded
    once.  Differentiable into all five tensors; under no_grad (or when nothing requires a
    gradient) nothing is saved.  For a fixed (N, H, value_head_splits(N, H)) the result is
    bit-reproducible and independent of h's row stride."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (h, w1, b1, w2, b2)):
        return _ValueHeadFn.apply(h, w1, b1, w2, b2, out_dtype)
    lead, N, H = _check(h, w1, b1, w2, b2, out_dtype)
    return _forward(h, w1, b1, w2, b2, out_dtype, lead, N, H)


class ValueHead(nn.Sequential):
    """make_head(n_embd, 1) of ppo_models.py:216-222 with the reference's modules and parameter
    names (0.weight, 0.bias, 2.weight, 2.bias, all bf16): its state_dict loads with strict=True.
    forward(h) returns [..., 1] bf16 like the reference (`.squeeze(-1)` call sites keep working);
    values(h) is the squeezed hot-path form in fp32 or bf16."""

    def __init__(self, n_embd: int):
        super().__init__(nn.Linear(n_embd, n_embd * 2).bfloat16(), nn.ReLU().bfloat16(),
                         nn.Linear(n_embd * 2, 1).bfloat16())
        self.n_embd = n_embd

    def values(self, h, out_dtype=torch.float32):
        return value_head(h, self[0].weight, self[0].bias, self[2].weight, self[2].bias, out_dtype)

    def forward(self, h):
        return self.values(h, torch.bfloat16).unsqueeze(-1)


def make_head(n_embd: int, out: int):
    """ppo_models.py:216-222.  out == 1 (the value head) is the fused ValueHead; any other width
    is the reference's bf16 nn.Sequential."""
    if out == 1:
        return ValueHead(n_embd)
    return nn.Sequential(nn.Linear(n_embd, n_embd * 2).bfloat16(), nn.ReLU().bfloat16(),
                         nn.Linear(n_embd * 2, out).bfloat16())
