"""Fused multi-tensor AdamW for MI355X — the counterpart of the three lines every update of the
reference ends with (accelerate_base_model.py:94-106, 263-265):

  FusedAdamW      torch.optim.AdamW's constructor, param_groups and state keys (step, exp_avg,
                  exp_avg_sq), so CosineAnnealingLR drives it unchanged and state_dicts move
                  between the two; one launch per dtype combination instead of torch's launch
                  train.  master_weights=True keeps an fp32 master per bf16 parameter.
  adamw_step      the functional form over lists of tensors.
  step(polyak=)   the ILQL target-head sync (post_backward_callback, ilql_models.py:161-181)
                  folded into the same pass: the target is updated from the parameter values
                  still in registers (ILQLHeads.step_and_sync).
  clip_grad_norm_ torch.nn.utils.clip_grad_norm_ (norm_type 2) — DeepSpeed's `gradient_clipping:
                  1.0` of the reference's launch config — as a device record {norm, coef,
                  nonfinite, sumsq}: Σ g² in fp64 over all tensors, no host sync.
  step(max_grad_norm=)
                  that clip folded into the update: the step reads the coefficient from the
                  record on the device and scales every gradient element as it loads it, so the
                  clip costs one more read of the gradients and .grad is never rewritten.

  state_dtype="param"
                  torch's own state layout: exp_avg and exp_avg_sq are zeros_like(p), bf16 for a
                  bf16 parameter, and every op of the update is rounded to bf16 as torch rounds
                  it — the optimizer the reference runs on its bf16 models, at 4 B of state per
                  parameter instead of 8 (trlx_adamw_step_ex).

Every element goes through torch's _single_tensor_adam ops in fp32, each rounded separately
(trlx_adamw_step in include/trlx_t5_amd.h).  exp_avg and exp_avg_sq are fp32 unless the caller
asks for bf16 ones (adamw_step with bf16 moments, FusedAdamW(state_dtype="param")).
"""
import ctypes
from itertools import chain
from typing import Optional, Sequence

import torch

from . import _lib
from .ilql_heads import UNSET as _UNSET, check_polyak_pairs, polyak_update

__all__ = ["FusedAdamW", "adamw_step", "clip_grad_norm_", "schedule_table"]

_DTYPES = (torch.float32, torch.bfloat16)


def _check_entry(i, p, g, m, v, master):
    if p.dtype not in _DTYPES:
        raise ValueError(f"tensor {i}: unsupported parameter dtype {p.dtype} (float32 / bfloat16)")
    if g.dtype not in _DTYPES:
        raise ValueError(f"tensor {i}: unsupported gradient dtype {g.dtype} (float32 / bfloat16)")
    if g.layout != torch.strided:
        raise ValueError(f"tensor {i}: sparse gradients are not supported")
    for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
        if t.dtype not in _DTYPES:
            raise ValueError(f"tensor {i}: {name} must be float32 or bfloat16, got {t.dtype}")
    if m.dtype != v.dtype:  # one of the two is bf16: name that one
        name, other = ("exp_avg", "exp_avg_sq") if m.dtype == torch.bfloat16 else ("exp_avg_sq", "exp_avg")
        raise ValueError(f"tensor {i}: {name} must be float32 as {other} is (or both bfloat16), got torch.bfloat16")
    if master is not None and master.dtype != torch.float32:
        raise ValueError(f"tensor {i}: master must be float32, got {master.dtype}")
    if m.dtype == torch.bfloat16:  # torch's layout for a bf16 parameter: everything bf16, no master
        if p.dtype != torch.bfloat16 or g.dtype != torch.bfloat16:
            raise ValueError(f"tensor {i}: bfloat16 exp_avg / exp_avg_sq need a bfloat16 parameter and gradient, "
                             f"got {p.dtype} and {g.dtype}")
        if master is not None:
            raise ValueError(f"tensor {i}: bfloat16 exp_avg / exp_avg_sq take no master")
    if master is not None and p.dtype != torch.bfloat16:
        raise ValueError(f"tensor {i}: a master is for a bfloat16 parameter, this one is {p.dtype}")
    for name, t in (("grad", g), ("exp_avg", m), ("exp_avg_sq", v), ("master", master)):
        if t is None:
            continue
        if tuple(t.shape) != tuple(p.shape):
            raise ValueError(f"tensor {i}: {name} has shape {tuple(t.shape)} but the parameter {tuple(p.shape)}")
        if t.device != p.device:
            raise ValueError(f"tensor {i}: {name} is on {t.device} but the parameter on {p.device}")
    for name, t in (("parameter", p), ("grad", g), ("exp_avg", m), ("exp_avg_sq", v), ("master", master)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"tensor {i}: {name} must be contiguous")


def _key(t):
    return (t.data_ptr(), tuple(t.shape), t.dtype, t.device)


def _fold(params, polyak):
    """(targets aligned with params, alpha, leftover targets, leftover sources): a source that
    is one of `params` gets its target updated inside the step, the others by polyak_update."""
    if polyak is None:
        return [None] * len(params), 0.0, [], []
    targets, sources, alpha = polyak
    targets, sources = list(targets), list(sources)
    check_polyak_pairs(targets, sources)
    _lib.require_cuda(*targets, *sources)
    where = {_key(p): i for i, p in enumerate(params) if p.numel()}
    aligned, rest_t, rest_s = [None] * len(params), [], []
    for t, s in zip(targets, sources):
        i = where.get(_key(s))
        if i is None or aligned[i] is not None:
            rest_t.append(t)
            rest_s.append(s)
        else:
            aligned[i] = t
    return aligned, float(alpha), rest_t, rest_s


RECORD_FLOATS = ctypes.sizeof(_lib.GradNormRecord) // 4  # the record as a float32 tensor


def _check_max_norm(max_norm, name="max_norm"):
    max_norm = float(max_norm)
    if max_norm != max_norm or max_norm < 0.0:
        raise ValueError(f"{name} must be >= 0 (inf: the norm is recorded, nothing is clipped), got {max_norm}")
    return max_norm


def _check_grads(grads):
    for i, g in enumerate(grads):
        if g.layout != torch.strided:
            raise ValueError(f"gradient {i}: sparse gradients are not supported")
        if g.dtype not in _DTYPES:
            raise ValueError(f"gradient {i}: unsupported gradient dtype {g.dtype} (float32 / bfloat16)")
        if not g.is_contiguous():
            raise ValueError(f"gradient {i}: must be contiguous")
    _lib.require_cuda(*grads)
    if len({g.device for g in grads}) > 1:
        raise ValueError("the global norm is taken on one device: the gradients live on several")


def _check_record(record, dev):
    if not (isinstance(record, torch.Tensor) and record.dtype == torch.float32 and record.numel() == RECORD_FLOATS
            and record.is_contiguous() and record.device == dev):
        raise ValueError(f"grad_norm_record must be a contiguous float32 tensor of {RECORD_FLOATS} elements on {dev}")
    return record


def _workspace_bytes(grads):
    numel = (ctypes.c_int64 * len(grads))(*[g.numel() for g in grads])
    return int(_lib.query("trlx_grad_norm_workspace_bytes", numel, len(grads)))


def _grad_norm(grads, max_norm, record, workspace, scale_in_place):
    """trlx_grad_norm over validated gradients of one device, on that device's current stream."""
    n = len(grads)
    a = _lib.GradNormArgs()
    a.count = n
    a.g = (ctypes.c_void_p * n)(*[_lib.ptr(g) for g in grads])
    a.g_dtype = (ctypes.c_int * n)(*[_lib.dtype_code(g) for g in grads])
    a.numel = (ctypes.c_int64 * n)(*[g.numel() for g in grads])
    a.max_norm = max_norm
    a.record, a.workspace = record.data_ptr(), workspace.data_ptr()
    a.workspace_bytes = workspace.numel() * workspace.element_size()
    a.scale_in_place = scale_in_place
    with torch.cuda.device(grads[0].device):
        _lib.call("trlx_grad_norm", ctypes.byref(a), _lib.stream_of(grads[0]))


def _nonfinite_error():
    # torch.nn.utils.clip_grad_norm_'s message
    return RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be "
                        "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                        "`error_if_nonfinite=False`")


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for the L2 norm: total_norm = sqrt(Σ over all gradients Σ g²),
    every gradient scaled in place by min(max_norm / (total_norm + 1e-6), 1) — fp32 ops rounded as
    torch rounds them on the device (a bf16 gradient: coefficient and product each rounded to bf16) — and total_norm returned as a 0-d
    fp32 tensor on the device.  Unlike torch, Σ g² is accumulated in fp64 in a fixed order (the
    norm is the fp64 one rounded once, finite wherever the true norm fits fp32), fp32 and bf16
    gradients go through the same launches, and nothing syncs with the host unless
    error_if_nonfinite=True, which reads the record's flag and raises torch's RuntimeError before
    any gradient is touched.  max_norm: >= 0; inf records the norm and leaves the gradients
    (ValueError otherwise).  norm_type other than 2 raises ValueError; `foreach` is accepted
    for the signature and ignored.  Gradients: contiguous, fp32 / bf16, on one ROCm device."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm = _check_max_norm(max_norm)
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_ takes the L2 norm only (norm_type=2.0), got {norm_type}")
    if len(grads) == 0:
        return torch.tensor(0.0)
    _check_grads(grads)
    dev = grads[0].device
    record = torch.zeros(RECORD_FLOATS, dtype=torch.float32, device=dev)
    workspace = torch.empty(_workspace_bytes(grads) // 8, dtype=torch.float64, device=dev)
    if error_if_nonfinite:
        _grad_norm(grads, max_norm, record, workspace, 0)
        if int(record.view(torch.int32)[2].item()):  # the one host sync
            raise _nonfinite_error()
        _grad_norm(grads, max_norm, record, workspace, 2)
    else:
        _grad_norm(grads, max_norm, record, workspace, 1)
    return record[0]


def _launch(entries, step, lr, beta1, beta2, eps, weight_decay, alpha, record=None, sched=None, table=None):
    """entries: (p, g, m, v, master or None, target or None), validated.  One trlx_adamw_step per
    (parameter dtype, gradient dtype, state dtype, device); with a clip record
    trlx_adamw_step_clipped; bf16 moments go through trlx_adamw_step_ex.
    sched (a device schedule record): the _dev entries, which read every scalar from it and
    ignore step ... alpha; table: the fp64 rates that record's advance reads, named so that the
    library can refuse tensors that overlap it."""
    groups = {}
    for e in entries:
        groups.setdefault((e[0].dtype, e[1].dtype, e[2].dtype, e[0].device), []).append(e)
    for (pd, gd, sd, dev), es in groups.items():
        n = len(es)

        def column(k):
            return (ctypes.c_void_p * n)(*[_lib.ptr(e[k]) for e in es])

        cols = [column(k) for k in range(6)]
        a = _lib.AdamwArgs()
        a.p_dtype, a.g_dtype, a.count = _lib.dtype_code(es[0][0]), _lib.dtype_code(es[0][1]), n
        a.p, a.g, a.m, a.v, a.master, a.target = cols
        a.numel = (ctypes.c_int64 * n)(*[e[0].numel() for e in es])
        a.step, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = int(step), lr, beta1, beta2, eps, weight_decay
        a.alpha = alpha
        if table is not None:
            a.lr_table, a.n_lr = table.data_ptr(), table.numel()
        with torch.cuda.device(dev):
            stream = _lib.stream_of(es[0][0])
            if sd == torch.bfloat16:
                _lib.call("trlx_adamw_step_ex", ctypes.byref(a), _lib.BF16, _lib.ptr(record), _lib.ptr(sched), stream)
            elif sched is not None and record is None:
                _lib.call("trlx_adamw_step_dev", ctypes.byref(a), sched.data_ptr(), stream)
            elif sched is not None:
                _lib.call("trlx_adamw_step_clipped_dev", ctypes.byref(a), record.data_ptr(), sched.data_ptr(), stream)
            elif record is None:
                _lib.call("trlx_adamw_step", ctypes.byref(a), stream)
            else:
                _lib.call("trlx_adamw_step_clipped", ctypes.byref(a), record.data_ptr(), stream)


def _check_hyper(lr, betas, eps, weight_decay):
    lr, (b1, b2), eps, wd = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= b1 < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {b1}")
    if not 0.0 <= b2 < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {b2}")
    if not 0.0 <= wd:
        raise ValueError(f"Invalid weight_decay value: {wd}")
    return lr, b1, b2, eps, wd


def adamw_step(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
               exp_avg_sqs: Sequence[torch.Tensor], *, step: int, lr: float, betas, eps: float, weight_decay: float,
               masters: Optional[Sequence[Optional[torch.Tensor]]] = None, polyak=None,
               max_grad_norm: Optional[float] = None, grad_norm_record: Optional[torch.Tensor] = None):
    """One AdamW update (decoupled decay) of every tensor, in place, `step` >= 1 being the number
    of this update (torch's state["step"] after its increment).  params: fp32 / bf16; grads:
    fp32 / bf16; exp_avgs, exp_avg_sqs: all fp32, or all bf16 — torch's state of a bf16 parameter:
    params and grads are then bf16, there are no masters and every op of the update is rounded
    to bf16 as torch.optim.AdamW rounds it; masters: None, or per tensor None or the fp32
    master of a bf16 parameter (the master is updated, the parameter is the master rounded to
    bf16).  polyak=(targets, sources, alpha): after the update, target <- alpha·source +
    (1 - alpha)·target as polyak_update writes it; a source that is one of `params` is synced
    inside the same launch.  Tensors are grouped by dtype combination and device: one launch per
    group and _lib.ADAMW_MAX_TENSORS tensors.  max_grad_norm: the update takes every gradient
    clipped by the global L2 norm of `grads` (clip_grad_norm_'s values, bit for bit) without
    writing the gradients; grad_norm_record, a float32 tensor of 8 elements on the device,
    receives {norm, coef, nonfinite (int32), -, sumsq (float64)} (None: a temporary).
    All tensors contiguous, on a ROCm device."""
    params, grads, exp_avgs, exp_avg_sqs = list(params), list(grads), list(exp_avgs), list(exp_avg_sqs)
    masters = [None] * len(params) if masters is None else list(masters)
    if not (len(params) == len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(masters)):
        raise ValueError(f"{len(params)} params but {len(grads)} grads, {len(exp_avgs)} exp_avgs, "
                         f"{len(exp_avg_sqs)} exp_avg_sqs, {len(masters)} masters")
    if int(step) != step or step < 1:
        raise ValueError(f"step must be an integer >= 1 (the number of this update), got {step}")
    lr, b1, b2, eps, wd = _check_hyper(lr, betas, eps, weight_decay)
    if max_grad_norm is not None:
        max_grad_norm = _check_max_norm(max_grad_norm, "max_grad_norm")
    elif grad_norm_record is not None:
        raise ValueError("grad_norm_record is written by the clip: give max_grad_norm too")
    for i, e in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs, masters)):
        _check_entry(i, *e)
        if e[2].dtype != exp_avgs[0].dtype:
            raise ValueError(f"tensor {i}: exp_avg is {e[2].dtype} but tensor 0's is {exp_avgs[0].dtype}; the moments "
                             "of one call are all float32 or all bfloat16")
    if polyak is not None:
        check_polyak_pairs(list(polyak[0]), list(polyak[1]))
    _lib.require_cuda(*params, *grads, *exp_avgs, *exp_avg_sqs, *masters)
    record = None
    if max_grad_norm is not None and grads:
        _check_grads(grads)
        dev = grads[0].device
        record = (torch.zeros(RECORD_FLOATS, dtype=torch.float32, device=dev) if grad_norm_record is None
                  else _check_record(grad_norm_record, dev))
    targets, alpha, rest_t, rest_s = _fold(params, polyak)
    if record is not None:
        workspace = torch.empty(_workspace_bytes(grads) // 8, dtype=torch.float64, device=record.device)
        _grad_norm(grads, max_grad_norm, record, workspace, 0)
    _launch(list(zip(params, grads, exp_avgs, exp_avg_sqs, masters, targets)), step, lr, b1, b2, eps, wd, alpha,
            record)
    if rest_t:
        polyak_update(rest_t, rest_s, alpha)


def schedule_table(make_scheduler, n_steps, lr):
    """The learning rates a torch scheduler sets for updates 1 .. n_steps, as a float64 CPU tensor
    for FusedAdamW(capturable=True, lr_schedule=...): make_scheduler(optimizer) -> scheduler (for
    example lambda o: CosineAnnealingLR(o, T, eta_min=...)) is run on a throw-away one-parameter
    torch.optim.SGD of learning rate `lr`, so the table is torch's own schedule bit for bit, for
    any scheduler, and the device needs no cos."""
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError(f"n_steps must be >= 1, got {n_steps}")
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=float(lr))
    sched = make_scheduler(opt)
    rates = []
    for _ in range(n_steps):
        rates.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
    return torch.tensor(rates, dtype=torch.float64)


SCHED_WORDS = ctypes.sizeof(_lib.AdamwSched) // 8  # the schedule record as an int64 tensor


def _lr_rates(schedule, what="lr_schedule"):
    rates = torch.as_tensor(schedule, dtype=torch.float64).detach().cpu().reshape(-1).clone()
    if rates.numel() < 1:
        raise ValueError(f"{what} must hold at least one learning rate")
    if not bool(torch.isfinite(rates).all()) or bool((rates < 0).any()):
        raise ValueError(f"{what} must hold finite learning rates >= 0")
    return rates


def _is_table(x):
    return isinstance(x, (list, tuple)) or (isinstance(x, torch.Tensor) and x.dim() >= 1)


def _check_schedule(schedule, n_groups):
    """lr_schedule as validated rates: ("shared", rates) or ("per_group", [rates, ...]).  One
    table for every group: a sequence of numbers (0-d tensors count as numbers) or a 1-D tensor.
    One table per group: a sequence of sequences / 1-D tensors, or a 2-D tensor."""
    if isinstance(schedule, torch.Tensor):
        if schedule.dim() > 2:
            raise ValueError(f"lr_schedule: a tensor of {schedule.dim()} dimensions (1: one table, 2: one per group)")
        per_group = schedule.dim() == 2
    elif isinstance(schedule, (list, tuple)):
        kinds = {_is_table(x) for x in schedule}
        if len(kinds) > 1:
            raise ValueError("lr_schedule mixes learning rates and tables: give one table, or one table per group")
        per_group = kinds == {True}
    else:
        raise ValueError(f"lr_schedule must be a sequence or a tensor of learning rates, got {type(schedule).__name__}")
    if not per_group:
        if isinstance(schedule, (list, tuple)):
            schedule = [float(x) for x in schedule]
        return "shared", _lr_rates(schedule)
    if len(schedule) != n_groups:
        raise ValueError(f"lr_schedule holds {len(schedule)} tables for {n_groups} param groups")
    return "per_group", [_lr_rates(t, f"lr_schedule[{i}]") for i, t in enumerate(schedule)]


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW on the fused kernel.  Same constructor arguments (lr, betas, eps,
    weight_decay), param_groups and state keys (step: a CPU scalar tensor, exp_avg, exp_avg_sq),
    so lr schedulers drive it unchanged and a torch.optim.AdamW.state_dict() loads into it and
    the other way round.  exp_avg and exp_avg_sq are fp32 whatever the parameter's dtype
    (state_dtype="float32", the default).
    state_dtype="param" (keyword only): the state is torch.zeros_like(p) as in torch.optim.AdamW —
    bf16 moments for a bf16 parameter, updated with every op rounded to bf16 as torch rounds it
    (include/trlx_t5_amd.h, trlx_adamw_step_ex); fp32 parameters are unaffected.  A bf16
    parameter then needs a bf16 .grad (ValueError at step()), master_weights=True is refused by
    the constructor (ValueError), load_state_dict takes bf16 moments as saved and rounds fp32
    ones to bf16 once, and state_dict() loads into torch.optim.AdamW over the same parameters
    with nothing converted.  This reproduces torch's precision, bf16 exp_avg_sq standing still
    once (1 - beta2)·g² is below half its ulp included; it is not more accurate than fp32 state.
    master_weights=True keeps an fp32 `master` state per bf16 parameter (absent for fp32
    parameters): the master takes the update, the parameter is the master rounded to bf16.
    A parameter whose .grad is None is skipped and its step does not advance.  amsgrad,
    maximize, sparse gradients and complex parameters raise ValueError.
    max_grad_norm (keyword only; None: no clipping) is the default of step(max_grad_norm=): the
    global L2 norm over every parameter that has a gradient, all param groups together, clips
    the update as clip_grad_norm_ followed by step() would — bit for bit in the parameters and
    the state — with one difference: .grad is left UNCLIPPED (the kernel scales each element as
    it reads it), so code that inspects .grad after the step sees the raw gradients.  It is an
    attribute of the optimizer, not a key of defaults / param_groups: the state_dict stays
    torch.optim.AdamW's.  After a clipped step, grad_norm and clip_coef are 0-d fp32 device
    views of the record (None before); reading them is the caller's only host sync.

    capturable=True (keyword only) keeps the step counter, the learning rate and the seven
    scalars of the update in a small device record per param group (trlx_adamw_sched), so that
    step() reads nothing on the host and one captured step() replays correctly under
    torch.cuda.graph: per group one trlx_adamw_advance launch, then the launches of the update,
    which read the record.  No host sync in step(), no allocation after the first call.
      state[p]["step"]  a 0-d int64 device view of the group's counter (torch's keys, as its own
                        capturable=True keeps a device step); load_state_dict takes a CPU or
                        device step, requires the parameters of a group to agree (ValueError)
                        and writes the value into the record.
      grad is None      ValueError: one counter per group cannot express per-parameter steps.
      lr_schedule       None: the rate is group["lr"], copied to the device only when it changed
                        since the last call (a host comparison; change it outside a capture).
                        Otherwise the per-update rates, entry k-1 for update k, the last entry
                        holding afterwards: a sequence of numbers or a 1-D tensor for every group,
                        or one such table per group (a sequence of them, or a 2-D tensor);
                        validated by the constructor (ValueError).  schedule_table() bakes any torch
                        scheduler into one.  group["lr"] is then not read.
      skip_nonfinite    an update whose global gradient norm is inf or NaN is skipped on the
                        device, as DeepSpeed's optimizer skips it: no parameter, state or target
                        is written, the counter and the lr index do not advance, skipped_steps
                        counts it.  Without max_grad_norm the norm is still taken (recorded,
                        nothing clipped).
      sync_every        step(polyak=) syncs the targets only on updates whose number is a
                        multiple of it, decided on the device (0: every call syncs, as without
                        capturable); every source must then be stepped in the call (ValueError).
                        The same holds with skip_nonfinite: a source outside the step would be
                        synced by the host even on an update the device skipped.
      applied_steps, skipped_steps, last_lr
                        0-d device views of the record (int64, int64, float64): the view itself
                        with one param group, a list of one view per group with several.
    The bias corrections come from a product chain instead of pow() (include/trlx_t5_amd.h,
    trlx_adamw_advance): the fp32 scalars were those of the default mode bit for bit on every
    step number measured (1..10000), which is not a guarantee.  skip_nonfinite,
    sync_every or lr_schedule without capturable raise ValueError."""

    max_grad_norm = None
    grad_norm = None
    clip_coef = None
    _clip_buffers = None  # (record, workspace), allocated by the first clipped step

    state_dtype = "float32"
    capturable = False
    skip_nonfinite = False
    sync_every = 0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, master_weights=False, max_grad_norm=None, capturable=False, lr_schedule=None,
                 skip_nonfinite=False, sync_every=0, state_dtype="float32"):
        if isinstance(lr, torch.Tensor):
            lr = float(lr)
        _check_hyper(lr, betas, eps, weight_decay)
        if amsgrad:
            raise ValueError("FusedAdamW does not support amsgrad")
        if maximize:
            raise ValueError("FusedAdamW does not support maximize")
        if state_dtype not in ("float32", "param"):
            raise ValueError(f"state_dtype must be 'float32' or 'param', got {state_dtype!r}")
        if master_weights and state_dtype == "param":
            raise ValueError("state_dtype='param' keeps torch's bfloat16 state for a bfloat16 parameter; an fp32 "
                             "master (master_weights=True) goes with state_dtype='float32'")
        self.state_dtype = state_dtype
        # the keys of torch.optim.AdamW's groups, so the two state_dicts have one structure
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=bool(capturable), differentiable=False, fused=None,
                        decoupled_weight_decay=True)
        if int(sync_every) != sync_every or sync_every < 0:
            raise ValueError(f"sync_every must be an integer >= 0, got {sync_every}")
        if not capturable:
            for name, given in (("skip_nonfinite", skip_nonfinite), ("sync_every", sync_every),
                                ("lr_schedule", lr_schedule is not None)):
                if given:
                    raise ValueError(f"{name} is decided on the device: it needs capturable=True")
        self.capturable, self.skip_nonfinite, self.sync_every = bool(capturable), bool(skip_nonfinite), int(sync_every)
        self._lr_schedule = None  # set below, validated against the param groups
        self._sched = {}         # group index -> {"record", "table", "lr_host"}, made by the first step
        self._pending_step = {}  # group index -> a loaded step not yet written to a record
        self.master_weights = bool(master_weights)
        if max_grad_norm is not None:
            self.max_grad_norm = _check_max_norm(max_grad_norm, "max_grad_norm")
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                if p.is_complex():
                    raise ValueError("FusedAdamW does not support complex parameters")
        if lr_schedule is not None:
            self._lr_schedule = _check_schedule(lr_schedule, len(self.param_groups))

    def load_state_dict(self, state_dict):
        if self.state_dtype == "param" and any("master" in st for st in state_dict["state"].values()):
            raise ValueError("the checkpoint holds fp32 masters; state_dtype='param' keeps none")
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdamW does not support amsgrad / maximize (loaded param_groups)")
        if self.state_dtype == "param":
            # Optimizer.load_state_dict has cast every state tensor to its parameter's dtype, which
            # is this layout: bf16 moments are copied as saved, fp32 ones rounded to bf16 once (RNE)
            if self.capturable:
                self._load_steps()
            return
        # Optimizer.load_state_dict casts every state tensor to its parameter's dtype; exp_avg,
        # exp_avg_sq and master of a bf16 parameter are fp32 here: take them from the saved values
        saved = state_dict["state"]
        ids = chain.from_iterable(g["params"] for g in state_dict["param_groups"])
        ours = chain.from_iterable(g["params"] for g in self.param_groups)
        for pid, p in zip(ids, ours):
            if pid not in saved or p.dtype == torch.float32:
                continue
            for k in ("exp_avg", "exp_avg_sq", "master"):
                if k in saved[pid]:
                    self.state[p][k] = saved[pid][k].to(device=p.device, dtype=torch.float32, copy=True)
        if self.capturable:
            self._load_steps()

    def _load_steps(self):
        """Capturable mode after a load: one step per group, written into the group's record."""
        loaded = {}
        for gi, group in enumerate(self.param_groups):
            group["capturable"] = True
            steps = {int(float(self.state[p]["step"])) for p in group["params"]
                     if p in self.state and "step" in self.state[p]}
            if len(steps) > 1:
                raise ValueError(f"param group {gi}: the loaded parameters disagree on step ({sorted(steps)}); "
                                 "capturable mode keeps one counter per group")
            if steps:
                loaded[gi] = steps.pop()
        for gi, step in loaded.items():
            group = self.param_groups[gi]
            self._pending_step[gi] = step
            if group["params"] and all(p.is_cuda for p in group["params"]):
                view = self._sched_of(gi, group)["record"][0]
                for p in group["params"]:
                    if p in self.state and "step" in self.state[p]:
                        self.state[p]["step"] = view

    def _group_rates(self, gi):
        """The validated rates of group gi (None: follow group["lr"])."""
        if self._lr_schedule is None:
            return None
        kind, rates = self._lr_schedule
        if kind == "shared":
            return rates
        if gi >= len(rates):  # a group added after the constructor
            raise ValueError(f"lr_schedule holds {len(rates)} tables for {len(self.param_groups)} param groups")
        return rates[gi]

    def _sched_of(self, gi, group):
        """The group's device schedule record and lr table, allocated once."""
        sc = self._sched.get(gi)
        if sc is None:
            devs = {p.device for p in group["params"]}
            if len(devs) != 1:
                raise ValueError(f"param group {gi}: capturable mode needs the group's parameters on one device")
            dev = devs.pop()
            rates = self._group_rates(gi)
            record = torch.zeros(SCHED_WORDS, dtype=torch.int64, device=dev)
            if rates is None:
                lr_host = float(group["lr"])
                table = torch.tensor([lr_host], dtype=torch.float64).to(dev)
            else:
                lr_host, table = None, rates.to(dev)
            sc = self._sched[gi] = dict(record=record, table=table, lr_host=lr_host)
        if gi in self._pending_step:
            sc["record"][0] = self._pending_step.pop(gi)
        return sc

    def _views(self, pick):
        out = [pick(self._sched_of(gi, g)["record"]) for gi, g in enumerate(self.param_groups)]
        return out[0] if len(out) == 1 else out

    @property
    def applied_steps(self):
        return self._views(lambda r: r[0]) if self.capturable else None

    @property
    def skipped_steps(self):
        return self._views(lambda r: r[1]) if self.capturable else None

    @property
    def last_lr(self):
        return self._views(lambda r: r.view(torch.float64)[_lib.AdamwSched.lr.offset // 8]) if self.capturable else None

    def _init_state(self, p, step_view=None):
        state = self.state[p]
        if "step" not in state:
            state["step"] = torch.tensor(0.0, dtype=torch.float32) if step_view is None else step_view
            dtype = p.dtype if self.state_dtype == "param" else torch.float32
            state["exp_avg"] = torch.zeros_like(p, dtype=dtype, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(p, dtype=dtype, memory_format=torch.contiguous_format)
        if self.master_weights and p.dtype == torch.bfloat16 and "master" not in state:
            state["master"] = p.detach().to(torch.float32, memory_format=torch.contiguous_format, copy=True)
        return state

    def _clip_record(self, grads):
        """The cached record and workspace, (re)allocated only when the gradients need more."""
        dev, need = grads[0].device, _workspace_bytes(grads)
        buf = self._clip_buffers
        if buf is None or buf[0].device != dev or buf[1].numel() * 8 < need:
            record = torch.zeros(RECORD_FLOATS, dtype=torch.float32, device=dev)
            buf = self._clip_buffers = (record, torch.empty(need // 8, dtype=torch.float64, device=dev))
            self.grad_norm, self.clip_coef = record[0], record[1]
        return buf

    @torch.no_grad()
    def step(self, closure=None, *, polyak=None, max_grad_norm=_UNSET):
        """One update of every parameter that has a gradient.  polyak=(targets, sources, alpha):
        the Polyak sync target <- alpha·source + (1 - alpha)·target after the update, bit for
        bit what step() followed by polyak_update(targets, sources, alpha) leaves; every source
        that is stepped in this call is synced inside the optimizer's launch, any other one by
        polyak_update.  max_grad_norm (default: the constructor's; None: no clipping): one
        global norm over all gradients of this call, then the clipped launches — no host sync,
        no allocation after the first clipped step, .grad left unclipped (see the class)."""
        if max_grad_norm is _UNSET:
            max_grad_norm = self.max_grad_norm
        if max_grad_norm is not None:
            max_grad_norm = _check_max_norm(max_grad_norm, "max_grad_norm")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            self._step_capturable(polyak, max_grad_norm)
            return loss
        work = []  # (group, p, state), everything validated before any state changes
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdamW does not support amsgrad / maximize")
            _check_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("FusedAdamW does not support sparse gradients")
                if p.is_complex():
                    raise ValueError("FusedAdamW does not support complex parameters")
                _lib.require_cuda(p, p.grad)
                state = self._init_state(p)
                _check_entry(len(work), p, p.grad, state["exp_avg"], state["exp_avg_sq"], state.get("master"))
                work.append((group, p, state))
        targets, alpha, rest_t, rest_s = _fold([p for _, p, _ in work], polyak)
        record = None
        if max_grad_norm is not None and work:
            grads = [p.grad for _, p, _ in work]
            _check_grads(grads)
            record, workspace = self._clip_record(grads)
            _grad_norm(grads, max_grad_norm, record, workspace, 0)
        buckets = {}  # one launch set per (group, step number): the scalars are per launch
        for (group, p, state), target in zip(work, targets):
            state["step"] += 1
            k = (id(group), int(state["step"].item()))
            buckets.setdefault(k, (group, []))[1].append(
                (p, p.grad, state["exp_avg"], state["exp_avg_sq"], state.get("master"), target))
        for (_, step), (group, entries) in buckets.items():
            lr, b1, b2, eps, wd = _check_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])
            _launch(entries, step, lr, b1, b2, eps, wd, alpha, record)
        if rest_t:
            polyak_update(rest_t, rest_s, alpha)
        return loss

    def _step_capturable(self, polyak, max_grad_norm):
        """step() with the counter, the rate and the scalars on the device: nothing is read on
        the host, and after the first call nothing is allocated."""
        groups = [(gi, g) for gi, g in enumerate(self.param_groups) if g["params"]]
        for gi, group in groups:  # every refusal before any state changes
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdamW does not support amsgrad / maximize")
            _check_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])
            for p in group["params"]:
                if p.grad is None:
                    raise ValueError(f"param group {gi}: a parameter has no gradient; capturable mode keeps one "
                                     "step counter per group and cannot skip a single parameter")
                if p.grad.is_sparse:
                    raise ValueError("FusedAdamW does not support sparse gradients")
                if p.is_complex():
                    raise ValueError("FusedAdamW does not support complex parameters")
        if polyak is not None and (self.sync_every > 0 or self.skip_nonfinite):
            stepped = {_key(p) for _, g in groups for p in g["params"] if p.numel()}
            for s in polyak[1]:
                if _key(s) in stepped:
                    continue
                if self.sync_every > 0:
                    raise ValueError("sync_every > 0: every polyak source must be a parameter stepped in this call "
                                     "(the cadence is decided on the device; a source outside the step would need "
                                     "a host branch)")
                raise ValueError("skip_nonfinite: every polyak source must be a parameter stepped in this call "
                                 "(whether the update is skipped is decided on the device; a source outside the "
                                 "step would be synced by the host even on a skipped update)")
        work = []  # (group index, p, state)
        for gi, group in groups:
            for p in group["params"]:
                _lib.require_cuda(p, p.grad)
            view = self._sched_of(gi, group)["record"][0]
            for p in group["params"]:
                state = self._init_state(p, view)
                _check_entry(len(work), p, p.grad, state["exp_avg"], state["exp_avg_sq"], state.get("master"))
                work.append((gi, p, state))
        targets, alpha, rest_t, rest_s = _fold([p for _, p, _ in work], polyak)
        if rest_t and (self.sync_every > 0 or self.skip_nonfinite):  # a source listed twice
            raise ValueError("sync_every > 0 / skip_nonfinite: a polyak source can be synced into one target only")
        record = None
        if (max_grad_norm is not None or self.skip_nonfinite) and work:
            grads = [p.grad for _, p, _ in work]
            _check_grads(grads)
            record, workspace = self._clip_record(grads)
            _grad_norm(grads, float("inf") if max_grad_norm is None else max_grad_norm, record, workspace, 0)
        sync_every = self.sync_every if self.sync_every > 0 else int(polyak is not None)
        for gi, group in groups:
            sc = self._sched_of(gi, group)
            lr, b1, b2, eps, wd = _check_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])
            if sc["lr_host"] is not None and sc["lr_host"] != lr:  # no schedule table: follow group["lr"]
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("group['lr'] changed inside a graph capture: change it outside, or give "
                                       "lr_schedule")
                sc["table"].copy_(torch.tensor([lr], dtype=torch.float64))
                sc["lr_host"] = lr
            a = _lib.AdamwAdvanceArgs()
            a.sched, a.lr_table, a.n_lr = sc["record"].data_ptr(), sc["table"].data_ptr(), sc["table"].numel()
            a.beta1, a.beta2, a.eps, a.weight_decay, a.alpha = b1, b2, eps, wd, alpha
            a.sync_every = sync_every
            a.grad_record = record.data_ptr() if (record is not None and self.skip_nonfinite) else None
            a.skip_nonfinite = int(self.skip_nonfinite)
            with torch.cuda.device(sc["record"].device):
                _lib.call("trlx_adamw_advance", ctypes.byref(a), _lib.stream_of(sc["record"]))
            entries = [(p, p.grad, st["exp_avg"], st["exp_avg_sq"], st.get("master"), t)
                       for (g2, p, st), t in zip(work, targets) if g2 == gi]
            _launch(entries, 0, 0.0, b1, b2, eps, wd, alpha, record if max_grad_norm is not None else None,
                    sched=sc["record"], table=sc["table"])
        if rest_t:
            polyak_update(rest_t, rest_s, alpha)
