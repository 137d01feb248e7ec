"""The projections of a T5 decoder layer's decode step with their neighbours in the same launch
(opt-in; csrc/t5_decode_linear.hip, trlx_t5_decode_linear).

  t5_decode_linear       out = epilogue(prologue(x) @ weight.T): the RMSNorm in front of a projection,
                         and behind it the residual add or the (gated) feed-forward activation
  T5DecodeBlockWeights   one decoder block's weights from HF's state_dict names, `qkv` and `wi` packed
  t5_decode_layer_fused  a decoder layer's decode step in 8 launches instead of 12

At decode shapes (B <= 256 rows, weights of 1-6 MB) a layer's time is its launch count, not its bytes.
The 12-launch layer is six torch.matmul projections, three t5_add_rmsnorm, t5_ff_act_packed and the
two attentions; here the three norms, the three adds and the activation ride in five projection
launches: [norm->qkv], self-attention, [o + residual -> h], [norm->cq], cross-attention,
[co + residual -> h], [norm->wi->act], [wo + residual -> h].

Rounding against the 12-launch layer: the normed rows carry the same bits as t5_rmsnorm's (they are
never written); the residual sum is bf16(acc_fp32 + h) instead of bf16(bf16(acc) + h), and the gated
activation reads the fp32 accumulators instead of their bf16 roundings -- one rounding fewer each;
the fp32 sums of a projection are added in this kernel's own fixed order, not hipBLASLt's.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from .t5_ff import ACTS, _act_code, _torch_ff_act, t5_ff_act
from .t5_norm import _torch_rmsnorm, t5_rmsnorm

__all__ = ["t5_decode_linear", "T5DecodeBlockWeights", "t5_decode_layer_fused", "geometry", "rows_geometry", "COLS_PER_BLOCK",
           "K_PER_CHUNK", "MAX_K", "NORM_MAX_K", "ROWS_PER_BLOCK", "MAX_M_LIVE"]

# the kernel's grid (csrc/t5_decode_linear.hip; trlx_t5_decode_linear_geometry reports it)
COLS_PER_BLOCK = 16     # N (F when gated) is a multiple of this
K_PER_CHUNK = 32        # K is a multiple of this
MAX_K = 16384
NORM_MAX_K = 8192       # with norm_weight: t5_rmsnorm's limit
# the rows form (csrc/t5_decode_linear_rows.hip; trlx_t5_decode_linear_rows_geometry reports it)
ROWS_PER_BLOCK = 32     # rows a workgroup owns with split_rows / live
MAX_M_LIVE = 4096       # the largest B the kernel takes with live


def geometry():
    """trlx_t5_decode_linear_geometry as a dict (needs no device)."""
    g = _lib.T5DecodeLinearGeometry()
    _lib.call("trlx_t5_decode_linear_geometry", ctypes.byref(g))
    return {n: getattr(g, n) for n, _ in g._fields_ if n != "reserved"}


def rows_geometry():
    """trlx_t5_decode_linear_rows_geometry as a dict (needs no device)."""
    g = _lib.T5DecodeLinearRowsGeometry()
    _lib.call("trlx_t5_decode_linear_rows_geometry", ctypes.byref(g))
    return {n: getattr(g, n) for n, _ in g._fields_ if n != "reserved"}


def _torch_decode_linear(x, weight, norm_weight, eps, residual, act, gated):
    """The same expression from the ops the fused call replaces: t5_rmsnorm, F.linear, the add,
    t5_ff_act on the device; their torch expressions where those refuse a tensor (bf16 / fp32 on a CPU)."""
    norm, ff = (t5_rmsnorm, t5_ff_act) if x.is_cuda else (_torch_rmsnorm, _torch_ff_act)
    y = x if norm_weight is None else norm(x, norm_weight, eps)
    z = F.linear(y, weight)
    if residual is not None:
        return residual + z
    if act is None:
        return z
    if gated:
        width = z.shape[-1] // 2
        return ff(z[..., :width], z[..., width:], act)
    return ff(z, None, act)


def _kernel_takes(x, weight, norm_weight, K, N):
    """The shapes and dtypes the kernel is built for; anything else on the list below is the torch route
    by design (fp32, K or N off the grid, a CPU tensor)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and K % K_PER_CHUNK == 0 and K_PER_CHUNK <= K <= MAX_K
            and N % COLS_PER_BLOCK == 0 and N >= COLS_PER_BLOCK and (norm_weight is None or K <= NORM_MAX_K))


def _ld(x2):
    return x2.stride(0) if x2.shape[0] > 1 else x2.shape[1]


def _on_grid(t):
    """A [rows, cols] view the kernel reads in place: unit element stride, 16-byte aligned base, a row
    stride that covers the row and is a multiple of 8 elements."""
    return (t.stride(1) == 1 and t.data_ptr() % 16 == 0 and
            (t.shape[0] == 1 or (t.stride(0) >= t.shape[1] and t.stride(0) % 8 == 0)))


def _check_live(who, live, B, device):
    if not isinstance(live, torch.Tensor) or live.dtype != torch.int64 or live.dim() != 1 or live.shape[0] != B \
            or live.device != device or not live.is_contiguous():
        got = f"{live.dtype} {tuple(live.shape)} on {live.device}" if isinstance(live, torch.Tensor) else type(live).__name__
        raise ValueError(f"{who}: live must be a contiguous int64 [{B}] on {device}, got {got}")


def _apply_dead_rows(got, live, r2):
    """The dead-row rule on a result computed for all rows: zeros, or the residual's row."""
    on = (live != 0)[:, None]
    return torch.where(on, got, torch.zeros_like(got) if r2 is None else r2.to(got.dtype))


def t5_decode_linear(x, weight, *, norm_weight=None, eps=1e-6, residual=None, act=None, gated=False, out=None,
                     live=None, split_rows=False):
    """out = epilogue(prologue(x) @ weight.T) in one launch, bf16 with fp32 accumulation.

    x: [B, K] or [B, 1, K]; rows K unit-stride elements one stride apart are read in place
    (h[:, -1, :]).  weight: [N, K], nn.Linear.weight as HF loads it ([2F, K] when gated: wi_0's rows,
    then wi_1's).
    norm_weight [K]: the projection takes t5_rmsnorm(x, norm_weight, eps) -- the same bits, never
    written.  At most one of: residual [B, N]: returns bf16(acc + residual), one rounding, and `out`
    may be the residual tensor itself (the stream updated in place); act in "relu" / "gelu_new" /
    "silu": returns act(acc), or act(u) * v with gated=True and u, v the accumulators of weight rows j
    and F + j, evaluated as t5_ff_act evaluates them.
    out: a preallocated [B, N] (F columns when gated) with unit element stride, so that a captured step
    allocates nothing; returned.  Without it a new tensor shaped like x with N columns.
    Forward only: an input that requires grad is refused.  Current stream, no host sync, no
    allocation beyond `out`, the same arguments at every token: the call can be captured.
    On a CPU device, or for a dtype or shape the kernel does not take by design (anything but bf16, K
    not a multiple of 32 or above 16384, above 8192 with norm_weight, N not a multiple of 16), the
    same expression runs as t5_rmsnorm, F.linear, the add, t5_ff_act.

    split_rows=True or a `live` takes trlx_t5_decode_linear_rows (csrc/t5_decode_linear_rows.hip): the
    rows spread over workgroups, ROWS_PER_BLOCK per workgroup, instead of every row in each.  A live
    row's result has the bits of the default call.  Opt-in: nothing here chooses by B.
    live: a contiguous int64 [B] on x's device, nonzero = live (the rollout recorder's `unfinished` as
    it is; B at most MAX_M_LIVE), read on the device, so the call stays the same launch at every token.  A dead row behaves
    as a zero input row and nothing of x is read for it: zeros in the plain, norm and act forms, the
    residual's row in the residual form, and left untouched when `out` is the residual.  The torch
    route computes every row and then applies the same rule.  As with the attentions' `live`, the
    skip is for a rollout sampled with score_finished=False, where nothing reads a finished row."""
    ts = [t for t in (x, weight, norm_weight, residual, out) if t is not None]
    if not all(isinstance(t, torch.Tensor) for t in ts):
        raise TypeError("t5_decode_linear: x, weight, norm_weight, residual and out must be tensors")
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise ValueError("t5_decode_linear is forward only: an input requires grad (use torch.no_grad(), or the "
                         "differentiable t5_rmsnorm / F.linear / t5_ff_act)")
    if act is not None:
        _act_code(act)
    if gated and act is None:
        raise ValueError("t5_decode_linear: gated=True needs an act")
    if act is not None and residual is not None:
        raise ValueError("t5_decode_linear: a residual and an act (one epilogue at most)")
    if x.dim() == 3 and x.shape[1] == 1:
        lead, x2 = (x.shape[0], 1), x[:, 0, :]
    elif x.dim() == 2:
        lead, x2 = (x.shape[0],), x
    else:
        raise ValueError(f"t5_decode_linear: x must be [B, K] or [B, 1, K], got {tuple(x.shape)}")
    B, K = x2.shape
    if weight.dim() != 2 or weight.shape[1] != K or weight.shape[0] < 1 or (gated and weight.shape[0] % 2):
        raise ValueError(f"t5_decode_linear: weight must be [{'2F' if gated else 'N'}, K = {K}], got {tuple(weight.shape)}")
    N = weight.shape[0] // 2 if gated else weight.shape[0]
    if B < 1:
        raise ValueError("t5_decode_linear: x has no rows")
    for name, t, shape in (("weight", weight, None), ("norm_weight", norm_weight, (K,)), ("residual", residual, (B, N)),
                           ("out", out, (B, N))):
        if t is None:
            continue
        if t.dtype != x.dtype or t.device != x.device:
            raise ValueError(f"t5_decode_linear: {name} must be {x.dtype} on {x.device}, got {t.dtype} on {t.device}")
        if shape is not None and tuple(t.shape if t.dim() != 3 else (t.shape[0], t.shape[2])) != shape:
            raise ValueError(f"t5_decode_linear: {name} must be {list(shape)}, got {tuple(t.shape)}")
    r2 = residual if residual is None or residual.dim() == 2 else residual[:, 0, :]
    o2 = out if out is None or out.dim() == 2 else out[:, 0, :]
    if o2 is not None and o2.stride(1) != 1:
        raise ValueError("t5_decode_linear: out must have unit element stride")
    if live is not None:
        _check_live("t5_decode_linear", live, B, x.device)

    if not _kernel_takes(x2, weight, norm_weight, K, N):
        got = _torch_decode_linear(x2, weight, norm_weight, eps, r2, act, gated)
        if live is not None:
            got = _apply_dead_rows(got, live, r2)
        if out is None:
            return got.view(*lead, N)
        o2.copy_(got)
        return out

    if not _on_grid(x2):
        x2 = x2.contiguous()
    if not _on_grid(weight):
        weight = weight.contiguous()
    if norm_weight is not None and (not norm_weight.is_contiguous() or norm_weight.data_ptr() % 16):
        norm_weight = norm_weight.contiguous().clone()
    if r2 is not None and not _on_grid(r2):
        if o2 is not None and r2.data_ptr() == o2.data_ptr():
            raise ValueError("t5_decode_linear: out is the residual, whose rows are off the kernel's grid (unit element "
                             "stride, 16-byte aligned, row stride a multiple of 8)")
        r2 = r2.contiguous()
    if o2 is None:
        out = torch.empty(*lead, N, dtype=x.dtype, device=x.device)
        o2 = out.view(B, N)
    elif not _on_grid(o2):
        raise ValueError("t5_decode_linear: out must be 16-byte aligned with a row stride that is a multiple of 8 elements")
    fields = dict(
        x=x2.data_ptr(), ld_x=_ld(x2), weight=weight.data_ptr(), ld_w=_ld(weight), norm_weight=_lib.ptr(norm_weight),
        residual=_lib.ptr(r2), ld_residual=N if r2 is None else _ld(r2), out=o2.data_ptr(), ld_out=_ld(o2),
        M=B, K=K, N=N, eps=float(eps), dtype=_lib.BF16, act=_lib.T5_ACT_NONE if act is None else ACTS[act],
        gated=int(bool(gated)))
    if live is not None or split_rows:
        args = _lib.T5DecodeLinearRowsArgs(live=_lib.ptr(live), reserved=0, **fields)
        _lib.call("trlx_t5_decode_linear_rows", ctypes.byref(args), _lib.stream_of(x2))
    else:
        args = _lib.T5DecodeLinearArgs(**fields)
        _lib.call("trlx_t5_decode_linear", ctypes.byref(args), _lib.stream_of(x2))
    return out


class T5DecodeBlockWeights:
    """One decoder block's weights for the 8-launch decode step, from HF's state_dict names under
    `prefix` (e.g. "decoder.block.3."):

      layer.0.SelfAttention.{q,k,v,o}.weight, layer.0.layer_norm.weight
      layer.1.EncDecAttention.{q,o}.weight,   layer.1.layer_norm.weight
      layer.2.DenseReluDense.{wi_0,wi_1,wo}.weight (gated) or {wi,wo}.weight, layer.2.layer_norm.weight

    Every tensor keeps nn.Linear.weight's [out, in] layout.  Built once: `qkv` [3 inner, D] (q's rows,
    k's, v's -- the output slices t5_decode_self_attention reads in place) and, gated, `wi` [2F, D]
    (wi_0's rows, then wi_1's).  EncDecAttention's k and v act on the encoder output once per rollout
    and are not part of a decode step.  A missing key raises KeyError with its full name."""

    SELF, CROSS, FF = "layer.0.SelfAttention.", "layer.1.EncDecAttention.", "layer.2.DenseReluDense."

    def __init__(self, qkv, o, cq, co, wi, wo, ln, gated):
        self.qkv, self.o, self.cq, self.co, self.wi, self.wo, self.ln, self.gated = qkv, o, cq, co, wi, wo, tuple(ln), gated
        self.inner = qkv.shape[0] // 3
        self.d_model = qkv.shape[1]
        self.d_ff = wi.shape[0] // 2 if gated else wi.shape[0]

    @classmethod
    def from_state_dict(cls, sd, prefix="", gated=True):
        def get(name):
            key = prefix + name
            if key not in sd:
                raise KeyError(f"T5DecodeBlockWeights: {key!r} is not in the state dict")
            return sd[key].detach()

        q, k, v = (get(cls.SELF + f"{n}.weight") for n in "qkv")
        if not (q.shape == k.shape == v.shape and q.dim() == 2):
            raise ValueError(f"T5DecodeBlockWeights: q, k, v must share one [inner, D] shape, got {tuple(q.shape)}, "
                             f"{tuple(k.shape)}, {tuple(v.shape)}")
        if gated:
            wi0, wi1 = get(cls.FF + "wi_0.weight"), get(cls.FF + "wi_1.weight")
            if wi0.shape != wi1.shape:
                raise ValueError(f"T5DecodeBlockWeights: wi_0 {tuple(wi0.shape)} and wi_1 {tuple(wi1.shape)} differ")
            wi = torch.cat([wi0, wi1], 0)
        else:
            wi = get(cls.FF + "wi.weight").contiguous()
        ln = [get(f"layer.{i}.layer_norm.weight").contiguous() for i in range(3)]
        return cls(torch.cat([q, k, v], 0), get(cls.SELF + "o.weight").contiguous(), get(cls.CROSS + "q.weight").contiguous(),
                   get(cls.CROSS + "o.weight").contiguous(), wi, get(cls.FF + "wo.weight").contiguous(), ln, bool(gated))

    def state_dict(self, prefix=""):
        """The rows back under HF's names (views of the packed tensors)."""
        i, f = self.inner, self.d_ff
        sd = {self.SELF + "q.weight": self.qkv[:i], self.SELF + "k.weight": self.qkv[i:2 * i],
              self.SELF + "v.weight": self.qkv[2 * i:], self.SELF + "o.weight": self.o,
              self.CROSS + "q.weight": self.cq, self.CROSS + "o.weight": self.co, self.FF + "wo.weight": self.wo}
        if self.gated:
            sd[self.FF + "wi_0.weight"], sd[self.FF + "wi_1.weight"] = self.wi[:f], self.wi[f:]
        else:
            sd[self.FF + "wi.weight"] = self.wi
        for n in range(3):
            sd[f"layer.{n}.layer_norm.weight"] = self.ln[n]
        return {prefix + k: v for k, v in sd.items()}


def t5_decode_layer_fused(h, w, self_attention, cross_attention, act="gelu_new", eps=1e-6, bufs=None, live=None,
                          split_rows=False):
    """One decoder layer's decode step on the residual stream h [B, D], updated in place, in 8 launches.

    w: T5DecodeBlockWeights.  self_attention(q, k_new, v_new) and cross_attention(q) are the caller's
    attention launches (t5_decode_self_attention with its cache, clock, bias table and live rows;
    t5_decode_cross_attention or its kv8 form) and return [B, inner].  bufs: None, or a dict with
    preallocated "qkv" [B, 3 inner], "cq" [B, inner] and "ff" [B, F] so that a captured step allocates
    nothing in the projections.
    live, split_rows: passed to the six projections (t5_decode_linear): the rows spread over workgroups,
    and with live=recorder.unfinished the rows that have finished skipped -- their qkv, cq and ff rows
    are zeros and their row of h is left as it was.  The attentions take their own `live`.  As theirs,
    the skip is for score_finished=False: a finished row's h is no longer the layer's output.
    Returns h."""
    bufs = bufs or {}
    i = w.inner
    kw = dict(live=live, split_rows=split_rows)
    qkv = t5_decode_linear(h, w.qkv, norm_weight=w.ln[0], eps=eps, out=bufs.get("qkv"), **kw)
    a = self_attention(qkv[:, :i], qkv[:, i:2 * i], qkv[:, 2 * i:])
    t5_decode_linear(a, w.o, residual=h, out=h, **kw)
    q = t5_decode_linear(h, w.cq, norm_weight=w.ln[1], eps=eps, out=bufs.get("cq"), **kw)
    c = cross_attention(q)
    t5_decode_linear(c, w.co, residual=h, out=h, **kw)
    f = t5_decode_linear(h, w.wi, norm_weight=w.ln[2], eps=eps, act=act, gated=w.gated, out=bufs.get("ff"), **kw)
    t5_decode_linear(f, w.wo, residual=h, out=h, **kw)
    return h
