"""Device-resident ILQL rollout store and offline experience builder — a drop-in for
trlx/pipeline/offline_pipeline.py `ILQLRolloutStorage`, trlx/data/ilql_types.py
`ILQLElement` and the tensor half of OfflineOrchestrator.make_experience
(trlx/orchestrator/offline_orchestrator.py:17-74).

The reference keeps Python lists of per-sample host tensors, pads them with six
`pad_sequence` calls per training batch in a DataLoader collate (offline_pipeline.py:88-108)
and copies the six results to the GPU (accelerate_ilql_model.py:58-68).  Here the dataset is
packed once into six flat buffers in HBM — ragged, with three int64 offset vectors
(L: input_ids / attention_mask, S: states_ixs / dones, A: actions_ixs / rewards), not the
PPO store's padded [capacity, W] buffers: the ILQL store is the whole static dataset, its
sample lengths vary widely and five of its six fields are int64, so a padded layout would be
mostly padding.  A training batch is ONE launch of `trlx_ilql_collate`, which pads while it
gathers, and equals the reference collate exactly (pad value 0, widths = the batch's longest
rows).  `from_samples` builds the five derived fields on the device
(`trlx_ilql_build_fields`); the host never holds them.

Out of scope: per-rank sharding of the loader (every rank iterates the whole store), and the
reference's printing of a decoded sample and of the mean reward / length.
"""
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ilql import ILQLBatch
from .modeling import moments
from .rollout_store import RolloutLoader

__all__ = ["ILQLElement", "ILQLRolloutStorage"]


@dataclass
class ILQLElement:
    """One offline sample (trlx/data/ilql_types.py:6-26)."""
    input_ids: torch.Tensor       # [L] int64
    attention_mask: torch.Tensor  # [L] int64
    rewards: torch.Tensor         # [A] fp32
    states_ixs: torch.Tensor      # [S] int64
    actions_ixs: torch.Tensor     # [A] int64
    dones: torch.Tensor           # [S] int64


_FIELDS = ("input_ids", "attention_mask", "rewards", "states_ixs", "actions_ixs", "dones")
_FAMILY = dict(input_ids="L", attention_mask="L", rewards="A", states_ixs="S", actions_ixs="A", dones="S")


def _lengths(ts, name):
    for i, t in enumerate(ts):
        if not torch.is_tensor(t) or t.dim() != 1:
            raise ValueError(f"{name}[{i}] must be a 1-D tensor")
    return np.fromiter((t.shape[0] for t in ts), dtype=np.int64, count=len(ts))


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off


def _pack(ts, dtype, device):
    """One concatenation and one upload; never an empty allocation (a family whose rows are all
    empty still hands the kernel a valid pointer)."""
    flat = torch.cat([t.reshape(-1) for t in ts]).to(device=device, dtype=dtype)
    return flat if flat.numel() else torch.zeros(1, dtype=dtype, device=device)


class ILQLRolloutStorage:
    """Rollout storage for ILQL training, resident in HBM (offline_pipeline.py:57-112).

    The constructor takes the reference's six lists of 1-D tensors (any device) and packs them
    once; `from_samples` is make_experience for tokenised samples.  `create_loader(batch_size)`
    yields ILQLBatch objects on the device; `store[i]` is an ILQLElement of views into the
    flat buffers."""

    def __init__(self, input_ids, attention_mask, rewards, states_ixs, actions_ixs, dones, device=None):
        lists = dict(input_ids=list(input_ids), attention_mask=list(attention_mask), rewards=list(rewards),
                     states_ixs=list(states_ixs), actions_ixs=list(actions_ixs), dones=list(dones))
        n = len(lists["input_ids"])
        if n == 0:
            raise ValueError("ILQLRolloutStorage: empty dataset")
        for f in _FIELDS:
            if len(lists[f]) != n:
                raise ValueError(f"ILQLRolloutStorage: {f} has {len(lists[f])} samples, input_ids has {n}")
        lens = {f: _lengths(lists[f], f) for f in _FIELDS}
        for a, b in (("attention_mask", "input_ids"), ("dones", "states_ixs"), ("rewards", "actions_ixs")):
            bad = np.nonzero(lens[a] != lens[b])[0]
            if bad.size:
                i = int(bad[0])
                raise ValueError(f"ILQLRolloutStorage: sample {i}: {a} has length {int(lens[a][i])}, "
                                 f"{b} has length {int(lens[b][i])}")
        device = self._device(device)
        flat = {f: _pack(lists[f], torch.float32 if f == "rewards" else torch.int64, device) for f in _FIELDS}
        self._init_flat(device, flat, lens["input_ids"], lens["states_ixs"], lens["actions_ixs"])

    @staticmethod
    def _device(device):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            raise ValueError("trlx_t5_amd: the ILQL store lives on a ROCm (cuda) device; there is no CPU path")
        return device

    def _init_flat(self, device, flat, len_L, len_S, len_A):
        self.device = device
        self._flat = flat
        self._len = {"L": len_L, "S": len_S, "A": len_A}  # host copies: batch widths need no device read
        self._off_host = {k: _offsets(v) for k, v in self._len.items()}
        self._off = {k: torch.from_numpy(v).to(device) for k, v in self._off_host.items()}
        self._n = len(len_L)

    @classmethod
    def from_samples(cls, input_ids: Sequence[torch.Tensor], rewards, prompt_lens=None, device=None):
        """make_experience (offline_orchestrator.py:17-74) for already tokenised samples:
        input_ids is a list of 1-D token tensors, rewards one scalar per sample, prompt_lens
        the prompt's token count per sample (None = 1, the bos-token case, :36-37).  The
        returns (r - mean) / (std + 1e-30) and the five derived fields are built on the
        device; the statistics are never read on the host.  One sample gives NaN returns, as
        the reference does.  Tokenising strings and locating `split_token` stay with the
        caller: prompt_lens[i] = len(tokenizer(s[:s.index(split_token) + len(split_token)]).input_ids)."""
        input_ids = list(input_ids)
        n = len(input_ids)
        if n == 0:
            raise ValueError("ILQLRolloutStorage: empty dataset")
        len_L = _lengths(input_ids, "input_ids")
        p = np.ones(n, dtype=np.int64) if prompt_lens is None else np.asarray(
            [int(v) for v in prompt_lens], dtype=np.int64)
        if p.shape != (n,):
            raise ValueError(f"ILQLRolloutStorage: {p.size} prompt lengths for {n} samples")
        bad = np.nonzero((p < 1) | (p >= len_L))[0]
        if bad.size:
            i = int(bad[0])
            raise ValueError(f"ILQLRolloutStorage: sample {i}: prompt length {int(p[i])} leaves no continuation "
                             f"in {int(len_L[i])} tokens (need 1 <= prompt length < sample length)")
        device = cls._device(device)
        raw = torch.as_tensor(rewards, dtype=torch.float32).reshape(-1).to(device)
        if raw.numel() != n:
            raise ValueError(f"ILQLRolloutStorage: {raw.numel()} rewards for {n} samples")
        self = cls.__new__(cls)
        len_A = len_L - p
        len_S = len_A + 1
        tot = {"L": int(len_L.sum()), "S": int(len_S.sum()), "A": int(len_A.sum())}
        flat = {f: torch.empty(tot[_FAMILY[f]], dtype=torch.float32 if f == "rewards" else torch.int64, device=device)
                for f in _FIELDS if f != "input_ids"}
        flat["input_ids"] = _pack(input_ids, torch.int64, device)
        self._init_flat(device, flat, len_L, len_S, len_A)
        st = moments(raw)
        p_dev = torch.from_numpy(p).to(device)
        _lib.call("trlx_ilql_build_fields", _lib.ptr(self._off["L"]), _lib.ptr(self._off["S"]),
                  _lib.ptr(self._off["A"]), _lib.ptr(p_dev), _lib.ptr(raw), _lib.ptr(st), n, tot["L"], tot["S"],
                  tot["A"], _lib.ptr(flat["attention_mask"]), _lib.ptr(flat["states_ixs"]),
                  _lib.ptr(flat["actions_ixs"]), _lib.ptr(flat["dones"]), _lib.ptr(flat["rewards"]),
                  _lib.stream_of(raw))
        return self

    def __len__(self) -> int:
        return self._n

    def __getitem__(self, index: int) -> ILQLElement:
        if not -self._n <= index < self._n:
            raise IndexError(index)
        i = index % self._n
        out = []
        for f in _FIELDS:
            off = self._off_host[_FAMILY[f]]
            out.append(self._flat[f][int(off[i]):int(off[i + 1])])
        return ILQLElement(*out)

    def device_bytes(self) -> int:
        """Bytes of HBM the packed dataset holds (six flat buffers + three offset vectors)."""
        return sum(t.numel() * t.element_size() for t in list(self._flat.values()) + list(self._off.values()))

    # -------------------------------------------------------------- collate
    def collate(self, idx: torch.Tensor, rows: np.ndarray) -> ILQLBatch:
        """Gather samples `idx` (device int64; `rows` = the same numbers on the host, any order,
        repeats allowed) into an ILQLBatch padded with 0 to the batch's longest rows, exactly
        the reference collate (offline_pipeline.py:88-108).  One launch."""
        _lib.require_cuda(idx)
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        n = len(rows)
        if idx.dtype != torch.int64 or idx.dim() != 1 or idx.shape[0] != n or idx.stride(0) != 1:
            raise ValueError(f"collate: idx must be a contiguous int64 vector of the {n} entries of rows")
        if n and (rows.min() < 0 or rows.max() >= self._n):
            raise IndexError(f"collate: sample numbers must lie in [0, {self._n})")
        w = {k: int(v[rows].max(initial=0)) for k, v in self._len.items()}
        out = {f: torch.empty((n, w[_FAMILY[f]]), dtype=self._flat[f].dtype, device=self.device) for f in _FIELDS}
        fl, off = self._flat, self._off
        _lib.call("trlx_ilql_collate", *[_lib.ptr(fl[f]) for f in _FIELDS], _lib.ptr(off["L"]), _lib.ptr(off["S"]),
                  _lib.ptr(off["A"]), self._n, _lib.ptr(idx), n, w["L"], w["S"], w["A"],
                  *[v for f in _FIELDS for v in (_lib.ptr(out[f]), out[f].stride(0))], _lib.stream_of(idx))
        return ILQLBatch(*[out[f] for f in _FIELDS])

    def create_loader(self, batch_size: int, shuffle: bool = True, generator: Optional[torch.Generator] = None,
                      drop_last: bool = False) -> RolloutLoader:
        """Batches of the stored samples in a torch.randperm order (the reference's loader
        always shuffles, offline_pipeline.py:110-112) or, for tests and evaluation,
        sequentially (shuffle=False)."""
        return RolloutLoader(self, batch_size, shuffle, generator, drop_last)
