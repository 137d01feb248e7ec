"""Shared pieces of the PPO sampling-step tests (csrc/ppo_sample.hip; used by
tests/test_gpu_ppo_sample.py and tests/test_gpu_ppo_sample_edges.py).

  oracle_keep / suppress   the fp64 restatement of the kept set defined in include/trlx_t5_amd.h
  run                      one ppo_sample_step call from CPU tensors (the wrapper)
  run_abi                  trlx_ppo_sample on device tensors as they are (row stride from
                           stride(0), no copies); the four outputs lie inside guard-filled buffers
  check_draw_and_logprob   the token's CDF interval holds u; logprob against fp64 log_softmax
  TABLE / need / select    the kernel's launch table (trlx_ppo_sample's `need`), restated
  thread_of / list_path    which thread holds an element, and whether the candidate list or the
                           block-wide search decides a row's thresholds, restated from the kernel
  place / row_split / LINE from ilql_sample_checks (the two kernels share common.h's row geometry)

Poison: the slack around placed logits rows holds +1e30, so a read outside a row changes the
result instead of faulting.  Test infrastructure only."""
import numpy as np
import torch

from trlx_t5_amd import _lib
import trlx_t5_amd as P
from ilql_sample_checks import DEV, LINE, LOGIT_POISON, place, row_split  # noqa: F401

NEG = float("-inf")
TOL = 1e-5
F32, BF16 = torch.float32, torch.bfloat16
GUARD = -7777
CAND_CAP, SEED = 512, 128   # ppo_sample.hip kPsCandCap, kPsSeed


# ------------------------------------------------------------------ fp64 oracle
def oracle_keep(x, T, top_k, top_p, min_keep=1):
    """x: fp64 [B, V] (eos already suppressed).  Returns (keep bool [B, V], w fp64 [B, V]):
    the kept set and exp(s - max s), s = x / T, for every finite entry."""
    B, V = x.shape
    keep = torch.isfinite(x)
    if top_k > 0:
        k = min(max(int(top_k), min_keep), V)
        kth = torch.topk(x, k, -1).values[:, -1:]
        keep = keep & (x >= kth)
    s = x / T
    smax = torch.where(keep, s, torch.full_like(s, NEG)).max(-1, keepdim=True).values
    w = torch.where(torch.isfinite(x), torch.exp(s - smax), torch.zeros_like(s))
    if top_p < 1.0:
        ws = torch.where(keep, w, torch.zeros_like(w))
        W = ws.sum(-1, keepdim=True)
        xs, order = torch.sort(torch.where(keep, x, torch.full_like(x, NEG)), -1, descending=True)
        wso = ws.gather(1, order)
        before = torch.cumsum(wso, -1) - wso            # mass ahead of each entry in sorted order
        first = torch.searchsorted(-xs, -xs, right=False)  # first entry of each run of ties = #(strictly greater)
        above = before.gather(1, first)                 # mass of the survivors strictly greater
        ok = (above <= top_p * W) | (first < min_keep)
        keep = keep & torch.zeros_like(keep).scatter(1, order, ok)
    return keep, w


def suppress(x, eos):
    x = x.double().clone()
    if eos is not None:
        x[:, eos] = NEG
    return x


# ------------------------------------------------------------------ the kernel
def run(logits, u, **kw):
    B = logits.shape[0]
    lg = logits.to(DEV)
    out = (torch.empty(B, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.float32, device=DEV),
           torch.empty(B, dtype=torch.float32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV))
    ids, lp = P.ppo_sample_step(lg, u=u.to(DEV, torch.float32), out=out, **kw)
    torch.cuda.synchronize()
    assert ids.data_ptr() == out[0].data_ptr() and lp.data_ptr() == out[1].data_ptr()
    return ids.cpu().reshape(B), lp.cpu(), out[2].cpu(), out[3].cpu()


OUT_DTYPES = (torch.int64, torch.float32, torch.float32, torch.int32)


def run_abi(lg, u, T=1.0, top_k=0, top_p=1.0, min_keep=1, cur_len=0, min_length=0, eos=None, pad=None,
            unfinished=None, dtype=None):
    """trlx_ppo_sample on device tensors as they are: lg [B, V] (row stride = stride(0), unit
    column stride), u fp32 [B], unfinished int64 [B] or None (updated in place).  The outputs lie
    8 elements inside buffers filled with GUARD, which must hold afterwards.  Synchronises;
    returns (ids, logprobs, min_kept, kept_count) on the CPU."""
    B, V = lg.shape
    assert lg.stride(1) == 1 and u.dtype == torch.float32 and u.is_contiguous() and u.device == lg.device
    bufs = [torch.full((B + 16,), GUARD, dtype=d, device=lg.device) for d in OUT_DTYPES]
    out = [b[8:8 + B] for b in bufs]
    _lib.call("trlx_ppo_sample", lg.data_ptr(), lg.stride(0) if B > 1 else V,
              _lib.dtype_code(lg) if dtype is None else dtype, B, V, float(T), int(top_k), float(top_p),
              int(min_keep), int(cur_len), int(min_length), -1 if eos is None else int(eos),
              -1 if pad is None else int(pad), u.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
              out[2].data_ptr(), out[3].data_ptr(), _lib.ptr(unfinished), _lib.stream_of(lg))
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:8] == GUARD).all()) and bool((b[8 + B:] == GUARD).all()), "a write outside the outputs"
    return tuple(o.cpu() for o in out)


def check_draw_and_logprob(logits, x, kept, w, ids, lp, u):
    """Token inside the kept set; its CDF interval over that set (index order) holds u within
    TOL; logprob = fp64 log_softmax of the unmodified row at the token."""
    B = x.shape[0]
    rows = torch.arange(B)
    assert bool(kept[rows, ids].all()), "token outside the kept set"
    pk = torch.where(kept, w, torch.zeros_like(w))
    cdf = torch.cumsum(pk / pk.sum(-1, keepdim=True), -1)
    hi = cdf[rows, ids]
    lo = hi - (pk / pk.sum(-1, keepdim=True))[rows, ids]
    ud = u.double()
    assert bool(((lo - TOL <= ud) & (ud <= hi + TOL)).all()), (lo, ud, hi)
    want = torch.log_softmax(logits.double(), -1)[rows, ids]
    torch.testing.assert_close(lp.double(), want, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ the launch table
# trlx_ppo_sample's launch table, (vectors per thread, threads) in the order it is walked
TABLE = {F32: [(1, 1024), (4, 1024), (8, 1024), (16, 512), (26, 512)],
         BF16: [(1, 1024), (4, 1024), (8, 512), (13, 512)]}


def esize(dtype):
    return 4 if dtype == F32 else 2


def need(V, epv, nt):
    """Vectors per thread that a row of V elements needs on nt threads (kLineVecs = LINE / 16)."""
    return (V // epv + 1 + (LINE // 16 - 1) + nt - 1) // nt


def select(V, dtype):
    """The table entry trlx_ppo_sample launches for V (None: refused)."""
    epv = 16 // esize(dtype)
    for n, nt in TABLE[dtype]:
        if need(V, epv, nt) <= n:
            return n, nt
    return None


def line_ld(V, dtype):
    """A row stride of whole 256-B lines: every row has row 0's head, tail and line shift."""
    es = esize(dtype)
    return ((V * es + LINE - 1) // LINE + 1) * LINE // es


# ------------------------------------------------------------------ the kernel's row layout and path
def thread_of(ptr, V, dtype, nt):
    """(thread, step) of every element of a row at byte address ptr: head element j -> thread j,
    tail element -> the last `tail` threads (step -1 for both), body vector i -> thread
    (i + shift) % nt at step (i + shift) / nt."""
    es = esize(dtype)
    epv = 16 // es
    head, nvec, tail0, tail, shift = row_split(ptr, V, es)
    j = torch.arange(V)
    slot = (j - head) // epv + shift
    thr, step = slot % nt, slot // nt
    thr[:head], step[:head] = torch.arange(head), -1
    thr[tail0:], step[tail0:] = nt - tail + torch.arange(tail), -1
    return thr, step


def _key16_floor(v):
    """The float whose order-preserving key is fkey(v) with the low 16 bits cleared: what the
    16-step bisection over the per-thread maxima returns for an n-th largest maximum v."""
    u = int(np.float32(v).view(np.uint32))
    k = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
    k &= 0xffff0000
    u = (k & 0x7fffffff) if k & 0x80000000 else (~k & 0xffffffff)
    return float(np.uint32(u).view(np.float32))


def list_path(x, keep, ptr, dtype, entry, top_k, top_p, min_keep):
    """Which search decides the thresholds of one row, restated from ppo_sample.hip (the code
    after `---- candidate list`): x fp32-exact values of the row [V] after eos suppression, keep
    the oracle's kept set.  Returns "none" (nothing to filter), "list" (the LDS candidate list
    decides), or why the block-wide searches run: "skipped" (n0 above the thread count or >= V,
    or no bound t0), "overflow" (more than 512 candidates), "smallest-kept" (top-p alone and the
    list's smallest value is kept)."""
    V = x.numel()
    nt = entry[1]
    k = 0 if top_k == 0 else min(max(top_k, min(min_keep, V)), V)
    if not (0 < k < V) and not top_p < 1.0:
        return "none"
    n0 = k if k > 0 else max(SEED, min(min_keep, V))
    if not (n0 <= nt and n0 < V):
        return "skipped"
    thr, _ = thread_of(ptr, V, dtype, nt)
    tmax = torch.full((nt,), NEG, dtype=torch.float64).scatter_reduce(0, thr, x.double(), "amax")
    v = float(torch.sort(tmax, descending=True).values[n0 - 1])
    if v == NEG:
        return "skipped"
    t0 = _key16_floor(v)
    cand = x[x >= t0]
    if cand.numel() > CAND_CAP:
        return "overflow"
    if k == 0 and bool(keep[x == cand.min()].any()):
        return "smallest-kept"
    return "list"
