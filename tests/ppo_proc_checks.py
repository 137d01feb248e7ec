"""Shared pieces of the processing sampling step's tests (tests/test_ppo_proc_cpu.py,
tests/test_gpu_ppo_proc.py): trlx_ppo_sample_proc through sampling.ppo_sample_step(processors=,
prefix=) and directly.

  processed        the fp32 torch restatement, on CPU tensors, of steps 1-5 of the processed row
                   defined in include/trlx_t5_amd.h (HF 4.21's _get_logits_processor order):
                   repetition penalty, no-repeat n-gram, bad words, min-length eos, forced token
  forced_id        the wrapper's forced bos / eos decision for a cur_len
  GOLDEN_CASES     the cases of tests/golden/sample_processors.npz (written by
                   tests/golden/make_golden_sample_processors.py from transformers' own classes)
  golden_inputs    the rows and prefixes of those cases, from the seed

It composes with ppo_sample_checks.oracle_keep / check_draw_and_logprob, which take the
processed row.  Test infrastructure only."""
import itertools

import torch

NEG = float("-inf")

# ------------------------------------------------------------------ the fixture's cases
GOLDEN_V, GOLDEN_B, GOLDEN_SEED = 37, 4, 20260
GOLDEN_PREFIX_LENS = (0, 1, 3, 9)
GOLDEN_BAD_WORDS = [[7], [3, 9], [1, 2, 3]]
# (name, kwargs of processed()): each processor alone at every setting, then all together
GOLDEN_CASES = ([(f"rp{rp}", dict(rp=rp)) for rp in (1.3, 0.8)] +
                [(f"g{g}", dict(g=g)) for g in (1, 2, 3)] +
                [("bad", dict(bad_words=GOLDEN_BAD_WORDS))] +
                [(f"all-rp{rp}-g{g}", dict(rp=rp, g=g, bad_words=GOLDEN_BAD_WORDS))
                 for rp, g in itertools.product((1.3, 0.8), (1, 2, 3))] +
                [("forced-bos", dict(rp=1.3, g=2, bad_words=GOLDEN_BAD_WORDS, forced_bos=5)),
                 ("forced-eos", dict(rp=0.8, forced_eos=1, max_length=max(GOLDEN_PREFIX_LENS) + 1)),
                 ("forced-both", dict(forced_bos=5, forced_eos=1, max_length=2))])


def case_kwargs(kw, n):
    """processed()'s keywords for a GOLDEN_CASES entry at prefix length n (HF's cur_len): the
    forced bos / eos settings become the one forced id of that step."""
    kw = dict(kw)
    forced = forced_id(n, kw.pop("forced_bos", None), kw.pop("forced_eos", None), kw.pop("max_length", None))
    return dict(kw, forced=forced)


def golden_inputs():
    """(logits fp32 [B, V], {n: prefix int64 [B, n]}): rows of sigma 3 with a few exact zeros and
    -inf entries; prefixes drawn from 12 tokens so that tokens and n-grams repeat, with rows that
    end in the bad words' own prefixes ([3] and [1, 2])."""
    g = torch.Generator().manual_seed(GOLDEN_SEED)
    x = 3.0 * torch.randn(GOLDEN_B, GOLDEN_V, generator=g)
    x[0, 2] = 0.0
    x[1, 9] = NEG
    full = torch.randint(0, 12, (GOLDEN_B, max(GOLDEN_PREFIX_LENS)), generator=g)
    full[0, -3:] = torch.tensor([4, 1, 2])                   # ends with [1, 2]: bans 3
    full[1, -1] = 3                                          # ends with [3]: bans 9
    full[2] = torch.tensor([5, 6, 5, 6, 5, 6, 5, 6, 5])      # every 2- and 3-gram repeats
    full[3, :3] = torch.tensor([8, 8, 8])
    # a prefix of length n is the last n tokens, so every length ends the way the full one does
    return x, {n: full[:, full.shape[1] - n:].contiguous() for n in GOLDEN_PREFIX_LENS}


# ------------------------------------------------------------------ the oracle
def forced_id(cur_len, forced_bos=None, forced_eos=None, max_length=None):
    """bos at cur_len == 1, eos at cur_len == max_length - 1, eos wins; -1 = none."""
    if forced_eos is not None and cur_len == max_length - 1:
        return forced_eos
    if forced_bos is not None and cur_len == 1:
        return forced_bos
    return -1


def processed(logits, prefix, rp=1.0, g=0, bad_words=(), eos=None, forced=-1):
    """The processed row, fp32 [B, V] on the CPU.  logits: [B, V] (upcast to fp32 as they are);
    prefix: int64 [B, n] (HF's input_ids).  eos: suppressed (cur_len < min_length), or None.
    A prefix token outside [0, V) is no target of any processor; it keeps its position in the
    matches, which compare the values."""
    x = logits.detach().cpu().float().clone()
    B, V = x.shape
    rows = [[int(t) for t in r] for r in prefix.cpu().tolist()] if prefix.numel() else [[] for _ in range(B)]
    n = len(rows[0])
    for b, p in enumerate(rows):
        if rp != 1.0:
            idx = torch.tensor(sorted({t for t in p if 0 <= t < V}), dtype=torch.int64)
            s = x[b, idx]
            x[b, idx] = torch.where(s < 0, s * rp, s / rp)
        banned = set()
        if g > 0 and n + 1 >= g:
            tail = p[n - g + 1:]
            for i in range(n - g + 1):
                if p[i:i + g - 1] == tail:
                    banned.add(p[i + g - 1])
        for w in bad_words:
            k = len(w) - 1
            if n >= k and (k == 0 or p[n - k:] == list(w[:k])):
                banned.add(int(w[k]))
        for t in banned:
            if 0 <= t < V:
                x[b, t] = NEG
    if eos is not None:
        x[:, eos] = NEG
    if forced >= 0:
        x[:] = NEG
        x[:, forced] = 0.0
    return x


def finite_min_and_count(x):
    """(smallest finite entry fp32 [B], number of finite entries int32 [B]) of a processed row."""
    fin = torch.isfinite(x)
    return torch.where(fin, x, torch.full_like(x, float("inf"))).min(-1).values, fin.sum(-1).to(torch.int32)
