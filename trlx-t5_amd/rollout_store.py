"""Device-resident PPO rollout store — a drop-in for
trlx/pipeline/ppo_pipeline.py `PPORolloutStorage` and trlx/data/ppo_types.py.

The reference moves every experience chunk to the host (`.cpu()` of five tensors,
ppo_orchestrator.py:169-173), splits it into per-sample `PPORLElement`s (:177-186) and
re-pads them per training batch with `pad_sequence` in a DataLoader collate
(ppo_pipeline.py:36-66), then copies the batch back to the GPU
(accelerate_ppo_model.py:81-85).  Here the store keeps each field as a padded columnar
buffer in HBM — queries right-aligned (left-padded with pad_token_id), responses
left-aligned (right-padded with pad_token_id), logprobs / values / rewards left-aligned
(right-padded with 0.0) — so pushing a generation batch and collating a training batch are
each ONE launch of `trlx_rows_copy`, and a batch never leaves the device.  The collated
batch equals the reference collate exactly: the rows' own padding is already in place, so
padding a batch to its widest query / response is a column window of the buffers.
"""
import ctypes
from dataclasses import dataclass
from typing import Iterable, List, Optional

import numpy as np
import torch

from . import _lib

__all__ = ["PPORLElement", "PPORLBatch", "PPORolloutStorage", "PPORolloutRecorder", "RolloutLoader"]


@dataclass
class PPORLElement:
    """One rollout (trlx/data/ppo_types.py:6-31)."""
    query_tensor: torch.Tensor
    response_tensor: torch.Tensor
    logprobs: torch.Tensor
    values: torch.Tensor
    rewards: torch.Tensor


@dataclass
class PPORLBatch:
    """A collated batch (trlx/data/ppo_types.py:34-57)."""
    query_tensors: torch.Tensor
    response_tensors: torch.Tensor
    logprobs: torch.Tensor
    values: torch.Tensor
    rewards: torch.Tensor


_FIELDS = ("query", "response", "logprobs", "values", "rewards")


def _rows_copy(fields, rows, src_idx=None, src_row0=0, dst_idx=None, dst_row0=0, stream=None):
    """fields: list of (src, dst, src_col0, dst_col0, cols) with 2-D tensors (row stride =
    stride(0), unit column stride)."""
    n = len(fields)
    srcs = (ctypes.c_void_p * n)(*[f[0].data_ptr() for f in fields])
    dsts = (ctypes.c_void_p * n)(*[f[1].data_ptr() for f in fields])
    sld = (ctypes.c_int64 * n)(*[f[0].stride(0) for f in fields])
    dld = (ctypes.c_int64 * n)(*[f[1].stride(0) for f in fields])
    sc0 = (ctypes.c_int64 * n)(*[f[2] for f in fields])
    dc0 = (ctypes.c_int64 * n)(*[f[3] for f in fields])
    cols = (ctypes.c_int64 * n)(*[f[4] for f in fields])
    es = (ctypes.c_int * n)(*[f[0].element_size() for f in fields])
    for f in fields:
        if f[0].dtype != f[1].dtype or f[0].stride(-1) != 1 or f[1].stride(-1) != 1:
            raise ValueError("rows_copy: matching dtypes and unit column strides required")
    s = stream if stream is not None else _lib.stream_of(fields[0][1])
    _lib.call("trlx_rows_copy", n, ctypes.cast(srcs, ctypes.c_void_p), ctypes.cast(dsts, ctypes.c_void_p),
              ctypes.cast(sld, ctypes.c_void_p), ctypes.cast(dld, ctypes.c_void_p),
              ctypes.cast(sc0, ctypes.c_void_p), ctypes.cast(dc0, ctypes.c_void_p),
              ctypes.cast(cols, ctypes.c_void_p), ctypes.cast(es, ctypes.c_void_p), int(rows),
              _lib.ptr(src_idx), int(src_row0), _lib.ptr(dst_idx), int(dst_row0), s)


class PPORolloutStorage:
    """Rollout storage for PPO training, resident in HBM (ppo_pipeline.py:11-68).

    push(exps) takes the reference's iterable of PPORLElement; push_batch(...) takes a
    generation batch as [n, W] device tensors (the orchestrator's own layout, no split into
    elements).  create_loader(batch_size, shuffle) yields PPORLBatch objects on the device.
    """

    def __init__(self, pad_token_id: int, device=None, capacity: int = 1024):
        self.pad_token_id = int(pad_token_id)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._cap = max(1, int(capacity))
        self._n = 0
        self._wq = 0  # buffer widths (max over pushed rows)
        self._wr = 0
        self._qw: List[int] = []  # per-row widths (host copies: batch widths need no device sync)
        self._rw: List[int] = []
        self._bufs = None
        self._dtypes = None

    # -------------------------------------------------------------- storage
    def _alloc(self, cap, wq, wr, dtypes):
        q = torch.full((cap, wq), self.pad_token_id, dtype=torch.int64, device=self.device)
        r = torch.full((cap, wr), self.pad_token_id, dtype=torch.int64, device=self.device)
        lp, v, rw = (torch.zeros((cap, wr), dtype=dt, device=self.device) for dt in dtypes)
        return [q, r, lp, v, rw]

    def _ensure(self, extra, wq, wr, dtypes):
        need = self._n + extra
        if self._bufs is not None and need <= self._cap and wq <= self._wq and wr <= self._wr:
            return
        cap = self._cap
        while cap < need:
            cap *= 2
        wq, wr = max(wq, self._wq), max(wr, self._wr)
        new = self._alloc(cap, wq, wr, dtypes)
        if self._bufs is not None and self._n:
            old = self._bufs
            # queries stay right-aligned, the rest left-aligned
            _rows_copy([(old[0], new[0], 0, wq - self._wq, self._wq)]
                       + [(old[i], new[i], 0, 0, self._wr) for i in range(1, 5)], self._n)
        self._bufs, self._cap, self._wq, self._wr = new, cap, wq, wr

    def push_batch(self, query_tensors, response_tensors, logprobs, values, rewards):
        """Append n rollouts given as [n, Wq] / [n, Wr] device tensors (one launch)."""
        ts = [query_tensors, response_tensors, logprobs, values, rewards]
        _lib.require_cuda(*ts)
        n, wq = query_tensors.shape
        wr = response_tensors.shape[1]
        for t in ts[1:]:
            if t.dim() != 2 or t.shape[0] != n or t.shape[1] != wr:
                raise ValueError(f"response-side tensors must be [{n}, {wr}], got {tuple(t.shape)}")
        if self._dtypes is None:
            self._dtypes = tuple(t.dtype for t in ts[2:])
        q = query_tensors.to(device=self.device, dtype=torch.int64).contiguous()
        r = response_tensors.to(device=self.device, dtype=torch.int64).contiguous()
        rest = [t.to(device=self.device, dtype=dt).contiguous() for t, dt in zip(ts[2:], self._dtypes)]
        self._ensure(n, wq, wr, self._dtypes)
        b = self._bufs
        _rows_copy([(q, b[0], 0, self._wq - wq, wq), (r, b[1], 0, 0, wr)]
                   + [(src, b[2 + i], 0, 0, wr) for i, src in enumerate(rest)], n, dst_row0=self._n)
        self._qw.extend([wq] * n)
        self._rw.extend([wr] * n)
        self._n += n

    def push(self, exps: Iterable[PPORLElement]):
        """The reference's push(list of PPORLElement) (ppo_pipeline.py:22-23): runs of
        consecutive elements with equal widths are stacked and pushed as one batch."""
        exps = list(exps)
        i = 0
        while i < len(exps):
            e0 = exps[i]
            j = i + 1
            while (j < len(exps) and exps[j].query_tensor.shape == e0.query_tensor.shape
                   and exps[j].response_tensor.shape == e0.response_tensor.shape):
                j += 1
            grp = exps[i:j]
            dev = self.device
            self.push_batch(*[torch.stack([getattr(e, f).to(dev) for e in grp]) for f in
                              ("query_tensor", "response_tensor", "logprobs", "values", "rewards")])
            i = j

    def clear_history(self):
        self._n = 0
        self._qw, self._rw = [], []
        if self._bufs is not None:  # restore the padding for the next fill
            self._bufs[0].fill_(self.pad_token_id)
            self._bufs[1].fill_(self.pad_token_id)
            for t in self._bufs[2:]:
                t.zero_()

    def __len__(self) -> int:
        return self._n

    def __getitem__(self, index: int) -> PPORLElement:
        if not -self._n <= index < self._n:
            raise IndexError(index)
        i = index % self._n
        b = self._bufs
        wq, wr = self._qw[i], self._rw[i]
        return PPORLElement(b[0][i, self._wq - wq:], b[1][i, :wr], b[2][i, :wr], b[3][i, :wr], b[4][i, :wr])

    # -------------------------------------------------------------- collate
    def collate(self, idx: torch.Tensor, rows: np.ndarray) -> PPORLBatch:
        """Gather rows `idx` (device int64; `rows` = the same indices on the host) into a
        PPORLBatch padded exactly like the reference collate (ppo_pipeline.py:40-66)."""
        n = len(rows)
        qw = np.asarray(self._qw)[rows]
        rw = np.asarray(self._rw)[rows]
        wq, wr = int(qw.max()), int(rw.max())
        b = self._bufs
        out = [torch.empty((n, wq), dtype=torch.int64, device=self.device),
               torch.empty((n, wr), dtype=torch.int64, device=self.device)]
        out += [torch.empty((n, wr), dtype=t.dtype, device=self.device) for t in b[2:]]
        _rows_copy([(b[0], out[0], self._wq - wq, 0, wq)] + [(b[i], out[i], 0, 0, wr) for i in range(1, 5)], n,
                   src_idx=idx)
        return PPORLBatch(*out)

    def create_loader(self, batch_size: int, shuffle: bool, generator: Optional[torch.Generator] = None,
                      drop_last: bool = False) -> "RolloutLoader":
        """Batches of the stored rollouts (ppo_pipeline.py:34-68 / torch DataLoader order:
        sequential, or a torch.randperm permutation when shuffle)."""
        return RolloutLoader(self, batch_size, shuffle, generator, drop_last)


class PPORolloutRecorder:
    """The columnar [B, T] buffers of one rollout chunk, filled one column per decode step by the
    recording sampling step (sampling.ppo_sample_step(..., ref_logits=, recorder=), one launch of
    trlx_ppo_sample_record): what ppo_orchestrator.py:76-167 obtains from generate() plus a
    second, teacher-forced pass of the policy and the reference model over [B, T, V] logits.

      tokens [B, T] int64 (pad)        logprobs / ref_logprobs [B, T] fp32 (0)
      values [B, T] fp32 (0)           lengths [B] int64 (T)      unfinished [B] int64 (1)
      t: the next column

    Allocated once; a step allocates nothing here.  hot_path: a PPOHotPath of the same B and T —
    logprobs / ref_logprobs are then its own lp_old / ref_lp, so
    PPOHotPath.experience_from_logprobs() reads them with no copy.  reset() re-arms the
    recorder for the next chunk; push_to() hands the chunk to a PPORolloutStorage.

    clock: a T5DecodeClock of capacity T on the same device.  The recording step then reads the
    column from the clock on the device (trlx_ppo_sample_proc_dev): the same launch at every token,
    so a captured decode step replays.  The step does not touch `t` and does not advance the clock
    — the caller's step ends with clock.advance(); a step issued with the clock at or past T
    writes nothing.  reset() also resets the clock; sync_t() reads the clock once (a host sync)
    and sets t = min(clock.t, T) for push_to() and PPOHotPath.experience_from_logprobs()."""

    def __init__(self, B: int, T: int, device, pad_token_id: int, eos_token_id: Optional[int], hot_path=None,
                 clock=None):
        self.B, self.T = int(B), int(T)
        if self.B < 1 or self.T < 1:
            raise ValueError("PPORolloutRecorder needs B >= 1 and T >= 1")
        self.device = torch.device(device)
        if clock is not None:
            from .t5_decode import T5DecodeClock
            if not isinstance(clock, T5DecodeClock):
                raise ValueError("clock must be a T5DecodeClock")
            if clock.T != self.T:
                raise ValueError(f"the clock's capacity T = {clock.T} is not the recorder's T = {self.T}")
            cd, rd = clock.device, self.device
            if cd.type != rd.type or (cd.index or 0) != (rd.index or 0):
                raise ValueError(f"the clock is on {clock.device}, the recorder on {self.device}")
        self.clock = clock
        if pad_token_id is None:
            raise ValueError("PPORolloutRecorder needs pad_token_id (the token of a finished row)")
        self.pad_token_id = int(pad_token_id)
        self.eos_token_id = None if eos_token_id is None else int(eos_token_id)
        dev = self.device
        if hot_path is not None:
            if (hot_path.B, hot_path.T) != (self.B, self.T) or hot_path.device != dev:
                raise ValueError(f"hot path ({hot_path.B},{hot_path.T}) on {hot_path.device} does not match the "
                                 f"recorder ({self.B},{self.T}) on {dev}")
            self.logprobs, self.ref_logprobs = hot_path.lp_old, hot_path.ref_lp
        else:
            self.logprobs = torch.empty((self.B, self.T), dtype=torch.float32, device=dev)
            self.ref_logprobs = torch.empty((self.B, self.T), dtype=torch.float32, device=dev)
        self.hot_path = hot_path
        self.tokens = torch.empty((self.B, self.T), dtype=torch.int64, device=dev)
        self.values = torch.empty((self.B, self.T), dtype=torch.float32, device=dev)
        self.lengths = torch.empty(self.B, dtype=torch.int64, device=dev)
        self.unfinished = torch.empty(self.B, dtype=torch.int64, device=dev)
        self.t = 0
        self.reset()

    def reset(self):
        """Re-arm for the next chunk: column 0, every row live, the buffers' initial contents."""
        self.tokens.fill_(self.pad_token_id)
        self.logprobs.zero_()
        self.ref_logprobs.zero_()
        self.values.zero_()
        self.lengths.fill_(self.T)
        self.unfinished.fill_(1)
        self.t = 0
        if self.clock is not None:
            self.clock.reset()

    def sync_t(self):
        """With a clock: t = min(clock.t, T), one host read (it synchronises).  Returns t."""
        if self.clock is not None:
            self.t = min(max(self.clock.t, 0), self.T)
        return self.t

    def _step_inputs(self, logits, ref_logits, values, pad_token_id, eos_token_id, unfinished):
        """The recording step's argument checks (all before any launch) -> (pad, eos, unfinished)."""
        B, V = logits.shape
        if B != self.B:
            raise ValueError(f"logits have {B} rows, the recorder {self.B}")
        if self.clock is None and self.t >= self.T:
            raise ValueError(f"the recorder is full (t = {self.t} = T): reset() starts the next chunk")
        if logits.device != self.device:
            raise ValueError(f"logits on {logits.device}, the recorder on {self.device}")
        if not isinstance(ref_logits, torch.Tensor) or tuple(ref_logits.shape) != (B, V) or \
                ref_logits.dtype != logits.dtype or ref_logits.device != logits.device:
            raise ValueError(f"ref_logits must be [{B}, {V}] {logits.dtype} on {logits.device} like logits")
        if values is not None and (tuple(values.shape) != (B,) or not values.is_contiguous() or
                                   values.device != self.device or
                                   values.dtype not in (torch.float32, torch.bfloat16)):
            raise ValueError(f"values must be a contiguous fp32 / bf16 [{B}] tensor on {self.device}")
        if pad_token_id is not None and int(pad_token_id) != self.pad_token_id:
            raise ValueError(f"pad_token_id {pad_token_id} is not the recorder's ({self.pad_token_id})")
        if eos_token_id is not None and self.eos_token_id is not None and int(eos_token_id) != self.eos_token_id:
            raise ValueError(f"eos_token_id {eos_token_id} is not the recorder's ({self.eos_token_id})")
        eos = self.eos_token_id if eos_token_id is None else int(eos_token_id)
        return self.pad_token_id, eos, (self.unfinished if unfinished is None else unfinished)

    def push_to(self, store: "PPORolloutStorage", query_tensors, rewards):
        """One PPORolloutStorage.push_batch of the first t columns: queries [B, Wq], rewards
        [B, >= t] (PPOHotPath.rewards), responses / logprobs / values from the recorder."""
        t = self.t
        if t < 1:
            raise ValueError("nothing recorded yet")
        if rewards.dim() != 2 or rewards.shape[0] != self.B or rewards.shape[1] < t:
            raise ValueError(f"rewards must be [{self.B}, >= {t}], got {tuple(rewards.shape)}")
        store.push_batch(query_tensors, self.tokens[:, :t], self.logprobs[:, :t], self.values[:, :t],
                         rewards[:, :t])


class RolloutLoader:
    """Iterable of device batches over a snapshot of a store with __len__, .device and
    .collate(idx, rows): PPORLBatch objects of a PPORolloutStorage, ILQLBatch objects of an
    ILQLRolloutStorage (ilql_store.py)."""

    def __init__(self, store, batch_size: int, shuffle: bool,
                 generator: Optional[torch.Generator], drop_last: bool):
        self.store, self.batch_size, self.shuffle = store, int(batch_size), bool(shuffle)
        self.generator, self.drop_last = generator, drop_last

    def __len__(self):
        n = len(self.store)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.store)
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        order_dev = order.to(self.store.device, non_blocking=False)
        host = order.numpy()
        for k in range(len(self)):
            lo, hi = k * self.batch_size, min(n, (k + 1) * self.batch_size)
            yield self.store.collate(order_dev[lo:hi], host[lo:hi])
