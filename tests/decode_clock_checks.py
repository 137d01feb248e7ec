"""Shared pieces of the decode clock's tests (tests/test_decode_clock_cpu.py,
tests/test_gpu_decode_clock.py): the device record {t, T, cur_len0, overrun, ...} of
include/trlx_t5_amd.h, trlx_t5_decode_attn_dev and trlx_ppo_sample_proc_dev.

  clock_rule        the pure-Python restatement of what the device-clock sampling step derives
                    from the clock: live / dead, cur_len, the eos suppression, the forced token
  groups            NG of a k_t5_decode_attn instantiation (csrc/t5_decode_attn.hip): the kernel
                    walks the cached columns in strides of NG groups, two in flight
  self_t            the decode steps around those strides
  vectors_per_thread, sampler_branch, SAMPLER_BRANCHES, sampler_vocabs
                    the launch table of csrc/ppo_sample.hip and the smallest V that reaches each
                    of its rows

Every GPU comparison built on these is exact equality of the raw bits: the clock route and the
host route execute the same arithmetic.  Test infrastructure only."""
import torch

GUARD = -77.0
CLOCK_WORDS = 8


# ------------------------------------------------------------------ the clock's rule
def clock_rule(t, T, cur_len0, buffers_T=None, min_length=0, eos=-1, forced_bos=-1, forced_eos=-1, max_length=0):
    """What one device-clock sampling step does at clock {t, T, cur_len0}: dict(live, t, cur_len,
    suppress_eos, forced).  buffers_T: the T of the record buffers (default the clock's)."""
    lim = T if buffers_T is None else min(T, buffers_T)
    if not 0 <= t < lim:
        return dict(live=False)
    cur_len = cur_len0 + t
    if forced_eos >= 0 and cur_len == max_length - 1:
        forced = forced_eos
    elif forced_bos >= 0 and cur_len == 1:
        forced = forced_bos
    else:
        forced = -1
    return dict(live=True, t=t, cur_len=cur_len, suppress_eos=eos >= 0 and cur_len < min_length, forced=forced)


def attention_live(t, T, max_len):
    return 0 <= t < min(T, max_len)


# ------------------------------------------------------------------ the attention kernel's geometry
def groups(dtype, d_kv):
    """NG = waves * key rows per wave-wide load: 4 * (64 / (d_kv / elements per 16-byte vector))."""
    epv = 8 if dtype == torch.bfloat16 else 4
    return 4 * (64 // (d_kv // epv))


def self_t(dtype, d_kv, max_len):
    ng = groups(dtype, d_kv)
    return sorted({0, 1, ng - 1, ng, 2 * ng - 1, 2 * ng, 2 * ng + 1, max_len - 1})


# ------------------------------------------------------------------ the sampler's launch table
LINE_VECS = 16  # common.h kLineVecs
# (vectors per thread N, threads NT) in table order, csrc/ppo_sample.hip TRLX_PSMP
SAMPLER_BRANCHES = {
    torch.bfloat16: ((1, 1024), (4, 1024), (8, 512), (13, 512)),
    torch.float32: ((1, 1024), (4, 1024), (8, 1024), (16, 512), (26, 512)),
}


def vectors_per_thread(V, dtype, nt):
    epv = 8 if dtype == torch.bfloat16 else 4
    return (V // epv + 1 + (LINE_VECS - 1) + nt - 1) // nt


def sampler_branch(V, dtype):
    """Index of the first table row that holds a row of V entries, or None."""
    for i, (n, nt) in enumerate(SAMPLER_BRANCHES[dtype]):
        if vectors_per_thread(V, dtype, nt) <= n:
            return i
    return None


def sampler_vocabs(dtype, small=517):
    """`small` and, for every further table row that some V reaches, the smallest such V, as
    [(branch, V)].  (A row whose capacity does not exceed an earlier row's is never taken: the
    fp32 table's 16 x 512 holds no more than its 8 x 1024.)"""
    assert sampler_branch(small, dtype) == 0
    out, seen, V = [(0, small)], 0, small
    while True:
        V += 1
        b = sampler_branch(V, dtype)
        if b is None:
            return out
        if b > seen:
            out.append((b, V))
            seen = b
