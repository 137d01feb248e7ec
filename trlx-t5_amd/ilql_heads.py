"""Drop-in for the ILQL heads of trlx/model/nn/ilql_models.py (config 5) on MI355X.

  ILQLHeads                   ilql_models.py:119-181 (V head, Q heads, frozen target-Q heads)
  ilql_target_q_at_actions    the target heads' second Linear (:31-34, :156) evaluated only
                              at the action tokens a* = input_ids[b, 1 + actions_ixs[b, a]]
  polyak_update               _sync_target_q_heads (:161-168), one launch for all tensors
  ILQLHeads.step_and_sync     the optimizer step and that sync in one pass (optim.FusedAdamW)

ILQLConfig.loss reads ONE scalar per (b, a) from each target-Q tensor (tq_i[b, a, a*]); the
reference still builds both target heads over the whole vocabulary ([B·A, 2H] x [2H, V] each).
ILQLHeads.forward_for_loss keeps the first Linear + ReLU in torch and replaces the second by
a gathered row dot z[b, a, :] · W2[a*, :] + b2[a*] (trlx_ilql_tq_at_actions): the [B, A, V]
target tensors are never built, and ILQLConfig.loss takes the [B, A] values directly.
"""
import ctypes
from copy import deepcopy
from typing import Optional, Sequence

import torch
from torch import nn

from . import _lib

__all__ = ["ILQLHeads", "ilql_target_q_at_actions", "make_head", "polyak_update"]

UNSET = object()  # "the optimizer's own value" for a keyword whose None means something else


def make_head(n_embd: int, out: int):
    """ilql_models.py:31-34."""
    return nn.Sequential(nn.Linear(n_embd, n_embd * 2), nn.ReLU(), nn.Linear(n_embd * 2, out))


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def ilql_target_q_at_actions(zs, w2s, b2s, input_ids, actions_ixs):
    """out_i[b, a] = z_i[b, a, :] · W2_i[a*, :] + b2_i[a*], a* = input_ids[b, 1 + actions_ixs[b, a]].

    zs: one or two [B, A, K] tensors (a target head's post-ReLU hidden activations), w2s: as many
    [V, K] weights (nn.Linear layout) of the same dtype (fp32 / bf16), b2s: as many [V] biases
    or None (also: None for no bias at all); input_ids [B, L], actions_ixs [B, A] (int64).
    Returns a tuple of fp32 [B, A] tensors.  fp32 accumulation in an order fixed by (K, dtype):
    bit-reproducible, independent of B, A and of the rows' alignment.  An a* outside [0, V)
    gives NaN (as in ILQLConfig.loss).  No autograd: the target heads are frozen."""
    zs, w2s = _as_list(zs), _as_list(w2s)
    b2s = [None] * len(zs) if b2s is None else _as_list(b2s)
    nh = len(zs)
    if nh not in (1, 2) or len(w2s) != nh or len(b2s) != nh:
        raise ValueError("one or two target heads: as many z, W2 and b2 (or None) entries")
    _lib.require_cuda(*zs, *w2s, *b2s)
    if zs[0].dim() != 3 or w2s[0].dim() != 2:
        raise ValueError("z must be [B, A, K] and W2 [V, K]")
    B, A, K = zs[0].shape
    V = w2s[0].shape[0]
    dt = zs[0].dtype
    if dt not in (torch.float32, torch.bfloat16):
        raise TypeError(f"unsupported dtype {dt} (float32 / bfloat16)")
    if input_ids.dim() != 2 or input_ids.shape[0] != B or tuple(actions_ixs.shape) != (B, A):
        raise ValueError(f"input_ids must be [B, L] and actions_ixs [B, A] = [{B}, {A}], got "
                         f"{tuple(input_ids.shape)} and {tuple(actions_ixs.shape)}")
    if B == 0 or A == 0 or K == 0 or V == 0:
        raise ValueError("empty z / W2")
    L = input_ids.shape[1]
    dev = zs[0].device
    ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
    aix = actions_ixs.to(device=dev, dtype=torch.int64).contiguous()
    a = _lib.IlqlTqArgs()
    a.dtype, a.nh, a.B, a.L, a.A, a.K, a.V = _lib.dtype_code(zs[0]), nh, B, L, A, K, V
    a.input_ids, a.actions_ixs = ids.data_ptr(), aix.data_ptr()
    keep, outs = [], []
    for i, (z, w, b) in enumerate(zip(zs, w2s, b2s)):
        if tuple(z.shape) != (B, A, K) or tuple(w.shape) != (V, K) or (b is not None and tuple(b.shape) != (V,)):
            raise ValueError(f"head {i}: z {tuple(z.shape)}, W2 {tuple(w.shape)}, b2 "
                             f"{None if b is None else tuple(b.shape)} do not match [{B}, {A}, {K}], [{V}, {K}], [{V}]")
        if z.dtype != dt or w.dtype != dt or (b is not None and b.dtype != dt):
            raise TypeError("z, W2 and b2 must share one dtype")
        z = z.detach() if z.stride(-1) == 1 else z.detach().contiguous()
        w = w.detach() if w.stride(-1) == 1 else w.detach().contiguous()
        b = None if b is None else b.detach().contiguous()
        out = torch.empty((B, A), dtype=torch.float32, device=dev)
        a.z[i], (a.z_sb[i], a.z_st[i]) = z.data_ptr(), (z.stride(0), z.stride(1))
        a.w2[i], a.w2_ld[i] = w.data_ptr(), (w.stride(0) if V > 1 else K)
        a.b2[i], a.out[i] = _lib.ptr(b), out.data_ptr()
        keep += [z, w, b]
        outs.append(out)
    _lib.call("trlx_ilql_tq_at_actions", ctypes.byref(a), _lib.stream_of(zs[0]))
    return tuple(outs)


def check_polyak_pairs(targets, sources):
    """The argument checks of polyak_update (also those of the sync folded into
    FusedAdamW.step): as many targets as sources, each pair of one dtype (fp32 / bf16) and
    shape, contiguous."""
    if len(targets) != len(sources):
        raise ValueError(f"{len(targets)} targets but {len(sources)} sources")
    for i, (t, s) in enumerate(zip(targets, sources)):
        if t.dtype != s.dtype:
            raise ValueError(f"pair {i}: target is {t.dtype} but source is {s.dtype}")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"pair {i}: unsupported dtype {t.dtype} (float32 / bfloat16)")
        if tuple(t.shape) != tuple(s.shape):
            raise ValueError(f"pair {i}: target has shape {tuple(t.shape)} but source {tuple(s.shape)}")
        if not (t.is_contiguous() and s.is_contiguous()):
            raise ValueError(f"pair {i}: tensors must be contiguous")


def polyak_update(targets: Sequence[torch.Tensor], sources: Sequence[torch.Tensor], alpha: float):
    """target <- (alpha * source) + (1.0 - alpha) * target for every pair, in place, bit for bit
    what torch's `target.copy_((alpha * source) + (1.0 - alpha) * target)` writes
    (ilql_models.py:161-168) — one launch per dtype and _lib.POLYAK_MAX_TENSORS tensors instead of
    three elementwise launches and two temporaries per tensor.  Each pair must agree in dtype
    (fp32 / bf16) and shape and be contiguous; a source that overlaps its target is refused."""
    targets, sources = list(targets), list(sources)
    check_polyak_pairs(targets, sources)
    _lib.require_cuda(*targets, *sources)
    for dt in (torch.float32, torch.bfloat16):
        pairs = [(t, s) for t, s in zip(targets, sources) if t.dtype == dt]
        if not pairs:
            continue
        if len({t.device for t, _ in pairs} | {s.device for _, s in pairs}) != 1:
            raise ValueError("targets and sources must live on one device")
        n = len(pairs)
        src = (ctypes.c_void_p * n)(*[s.data_ptr() for _, s in pairs])
        dst = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in pairs])
        numel = (ctypes.c_int64 * n)(*[t.numel() for t, _ in pairs])
        _lib.call("trlx_polyak_update", src, dst, numel, n, _lib.dtype_code(pairs[0][0]), float(alpha),
                  _lib.stream_of(pairs[0][0]))


class ILQLHeads(nn.Module):
    """ILQLHeads (ilql_models.py:119-181): the reference's constructor and parameter names
    (v_head.{0,2}.*, q_heads.{i}.{0,2}.*, target_q_heads.{i}.{0,2}.*), so its state_dict loads
    with strict=True.  The trainable GEMMs stay nn.Linear (the CQL cross-entropy needs the Q
    heads' full [B, A, V] rows; the V head is tiny)."""

    def __init__(self, config, hidden_size: int, vocab_size: int):
        super().__init__()
        self.hidden_size = hidden_size
        self.vocab_size = vocab_size
        self.v_head = make_head(self.hidden_size, 1)
        self.config = config
        n_qs = 2 if self.config.two_qs else 1
        self.q_heads = nn.ModuleList(make_head(self.hidden_size, self.vocab_size) for _ in range(n_qs))
        self.target_q_heads = nn.ModuleList(deepcopy(q_head) for q_head in self.q_heads)
        for q_head in self.target_q_heads:
            q_head.requires_grad_(False)

    @staticmethod
    def _select(hs, states_ixs, actions_ixs):
        """hs rows at states_ixs / actions_ixs by advanced indexing (the reference's hs.gather
        with a [B, A, H] int64 index, which is never built here).  Padded actions_ixs repeat
        index 0: the backward is an accumulating index_put."""
        if states_ixs is None:
            return hs, hs
        rows = torch.arange(hs.shape[0], device=hs.device)[:, None]
        return hs[rows, states_ixs], hs[rows, actions_ixs]

    def forward(self, hs: torch.Tensor, states_ixs: Optional[torch.Tensor] = None,
                actions_ixs: Optional[torch.Tensor] = None):
        """The reference's (qs, target_qs, vs) with full [B, A, V] target rows — the drop-in
        for generate, which needs them (ilql_sample_step)."""
        states_hs, actions_hs = self._select(hs, states_ixs, actions_ixs)
        qs = tuple(q_head(actions_hs) for q_head in self.q_heads)
        target_qs = tuple(q_head(actions_hs) for q_head in self.target_q_heads)
        vs = self.v_head(states_hs)
        return qs, target_qs, vs

    def forward_for_loss(self, hs: torch.Tensor, input_ids: torch.Tensor, states_ixs: torch.Tensor,
                         actions_ixs: torch.Tensor):
        """(qs, target_qs_at_actions, vs) for ILQLConfig.loss: each target entry is the fp32
        [B, A] value of that head at the action token — first Linear + ReLU in torch, then
        the gathered row dot (ilql_target_q_at_actions), under no_grad — instead of a
        [B, A, V] tensor of which the loss reads one element per row."""
        states_hs, actions_hs = self._select(hs, states_ixs, actions_ixs)
        qs = tuple(q_head(actions_hs) for q_head in self.q_heads)
        vs = self.v_head(states_hs)
        with torch.no_grad():
            a_hs = actions_hs.detach()
            zs = [q_head[1](q_head[0](a_hs)) for q_head in self.target_q_heads]
            target_qs = ilql_target_q_at_actions(zs, [h[2].weight for h in self.target_q_heads],
                                                 [h[2].bias for h in self.target_q_heads], input_ids, actions_ixs)
        return qs, target_qs, vs

    def sync_target_q_heads(self):
        """One polyak_update over all target parameters with config.alpha
        (ilql_models.py:161-181).  The reference's DeepSpeed ZeRO-3 branch (gathering the
        partitioned parameters on rank 0 first) is out of scope: parameters must be whole."""
        targets = [p.data for h in self.target_q_heads for p in h.parameters()]
        sources = [p.data for h in self.q_heads for p in h.parameters()]
        polyak_update(targets, sources, self.config.alpha)

    def step_and_sync(self, opt, closure=None, *, max_grad_norm=UNSET):
        """opt.step() and sync_target_q_heads() in one pass (opt: a FusedAdamW over these heads'
        parameters): every Q parameter the optimizer steps updates its target from the value
        just formed, bit for bit what the two calls leave; a Q parameter without a gradient is
        synced by polyak_update.  For the updates on which post_backward_callback syncs
        (every steps_for_target_q_sync); the others call opt.step().  max_grad_norm= is passed
        on to FusedAdamW.step (the global-norm clip folded into the same update; left out, the
        optimizer's own max_grad_norm holds).  With FusedAdamW(capturable=True,
        sync_every=cfg.steps_for_target_q_sync) call this on every update: the device decides
        which ones sync, which replaces the reference's modulo on the host."""
        step_kw = {} if max_grad_norm is UNSET else {"max_grad_norm": max_grad_norm}
        targets = [p.data for h in self.target_q_heads for p in h.parameters()]
        sources = [p.data for h in self.q_heads for p in h.parameters()]
        return opt.step(closure, polyak=(targets, sources, self.config.alpha), **step_kw)
