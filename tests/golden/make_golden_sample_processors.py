"""Writes tests/golden/sample_processors.npz: the rows that transformers' own logits processors
return for the cases of tests/ppo_proc_checks.py (GOLDEN_CASES x GOLDEN_PREFIX_LENS), on fp32
CPU rows, chained in the order of generate's _get_logits_processor: RepetitionPenalty,
NoRepeatNGram, NoBadWords, ForcedBOSToken, ForcedEOSToken.  Key "<case>/n<prefix length>".

    python tests/golden/make_golden_sample_processors.py

tests/test_ppo_proc_cpu.py compares tests/ppo_proc_checks.processed with this file bit for bit
(and, where transformers is installed, with hf_rows() live)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ppo_proc_checks as C  # noqa: E402


def hf_rows(logits, prefix, rp=1.0, g=0, bad_words=(), forced_bos=None, forced_eos=None, max_length=None):
    """The chain of transformers' classes on (input_ids = prefix, scores = logits)."""
    from transformers.generation import logits_process as lp

    chain = []
    if rp != 1.0:
        chain.append(lp.RepetitionPenaltyLogitsProcessor(penalty=rp))
    if g > 0:
        chain.append(lp.NoRepeatNGramLogitsProcessor(g))
    if bad_words:
        chain.append(lp.NoBadWordsLogitsProcessor([list(w) for w in bad_words], eos_token_id=None))
    if forced_bos is not None:
        chain.append(lp.ForcedBOSTokenLogitsProcessor(forced_bos))
    if forced_eos is not None:
        chain.append(lp.ForcedEOSTokenLogitsProcessor(max_length, forced_eos, device="cpu"))
    x = logits.clone()
    for proc in chain:
        x = proc(prefix, x)
    return x


def main():
    x, prefixes = C.golden_inputs()
    out = {}
    for name, kw in C.GOLDEN_CASES:
        for n, p in prefixes.items():
            out[f"{name}/n{n}"] = hf_rows(x, p, **kw).numpy()
    path = os.path.join(HERE, "sample_processors.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "rows sets,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
