"""Shared pieces of the recording sampling step's tests (tests/test_gpu_ppo_record.py):
trlx_ppo_sample_record through sampling.ppo_sample_step(ref_logits=, recorder=).

  SHAPES            one V per live launch-table entry (ppo_sample_checks.select confirms it)
  plain / recorded  one step without / with a recorder on the same inputs
  ref_want          fp64 log_softmax of the reference rows, as the kernel sees them, at the tokens
  snapshot          the recorder's buffers on the CPU (for before / after comparisons)

Test infrastructure only."""
import torch

import trlx_t5_amd as P
from ppo_sample_checks import BF16, DEV, F32, select

# (dtype, launch-table entry, V): every entry the dispatch can reach, at its largest V unless
# the interval holds one of the two vocabularies the project runs (32128, 50257)
SHAPES = [(F32, (1, 1024), 4035), (F32, (4, 1024), 16323), (F32, (8, 1024), 32128), (F32, (26, 512), 50257),
          (BF16, (1, 1024), 8071), (BF16, (4, 1024), 32128), (BF16, (13, 512), 50257)]
for _d, _e, _v in SHAPES:
    assert select(_v, _d) == _e

RTOL, ATOL = 1e-5, 1e-6   # the project's fp32 bar


def dname(dtype):
    return "f32" if dtype == F32 else "bf16"


def outs(B):
    return (torch.empty(B, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.float32, device=DEV),
            torch.empty(B, dtype=torch.float32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV))


def plain(lg, u, unfinished, **kw):
    """ppo_sample_step without a recorder on a clone of `unfinished`: (ids, lp, min, cnt, unfinished)."""
    unf = None if unfinished is None else unfinished.clone()
    o = outs(lg.shape[0])
    P.ppo_sample_step(lg, u=u, out=o, unfinished=unf, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in o) + (None if unf is None else unf.cpu(),)


def recorded(rec, lg, ref, u, **kw):
    """The recording step into `rec` (its own unfinished vector): (ids, lp, min, cnt) on the CPU."""
    o = outs(lg.shape[0])
    ids, lp = P.ppo_sample_step(lg, u=u, out=o, ref_logits=ref, recorder=rec, **kw)
    torch.cuda.synchronize()
    assert ids.data_ptr() == o[0].data_ptr() and lp.data_ptr() == o[1].data_ptr()
    return tuple(t.cpu() for t in o)


def ref_want(ref, ids):
    """fp64 log_softmax(ref)[ids]: the rows upcast as they are (bf16 values are not re-rounded)."""
    r = ref.detach().cpu().double()
    return torch.log_softmax(r, -1)[torch.arange(r.shape[0]), ids.reshape(-1).cpu()]


def snapshot(rec):
    return {k: getattr(rec, k).cpu().clone() for k in ("tokens", "logprobs", "ref_logprobs", "values", "lengths",
                                                       "unfinished")}, rec.t


def same_snapshot(a, b):
    return a[1] == b[1] and all(torch.equal(a[0][k], b[0][k]) for k in a[0])
