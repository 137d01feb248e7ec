"""Generate tests/golden/ilql_store.npz from the REFERENCE's offline data path:
OfflineOrchestrator.make_experience (trlx/orchestrator/offline_orchestrator.py:17-74) and
ILQLRolloutStorage with its loader's collate_fn (trlx/pipeline/offline_pipeline.py:57-112).
Data only: the inputs, the six per-sample lists (flat arrays + lengths) and the batches the
reference's own collate_fn gives for fixed index lists — no code.

Cases
  a  tokenizer None (samples are token lists, prompt length 1); 12 samples whose lengths
     include 2, 3, 63, 64, 65 and 129
  b  a stand-in character-level tokenizer and a split_token, so prompt lengths differ
  c  one sample: the returns are NaN (torch's std() of one element)

The rewards are drawn as 3·N(0,1) + 1; the script asserts that the reference's fp32 returns
lie within rtol 1e-5 / atol 1e-6 of the fp64 evaluation of the same formula on the same fp32
rewards — the bar the GPU test holds the device-built returns to.

Like make_golden.py (whose reference loaders it uses) this runs only where the reference
checkout is present; `trlx.orchestrator` (whose real __init__ pulls in the trainers) is a
shell made here with an empty Orchestrator base and an identity register_orchestrator.

Run:  python tests/golden/make_golden_ilql_store.py
"""
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

from make_golden import _load, _shell, gen, load_ppo_pipeline, load_reference  # noqa: E402

FIELDS = ("input_ids", "attention_mask", "rewards", "states_ixs", "actions_ixs", "dones")
SPLIT = "=>"


def load_offline():
    load_reference()
    load_ppo_pipeline()  # the real trlx.data / trlx.pipeline packages
    _load("trlx.data.ilql_types", "trlx/data/ilql_types.py")
    pipe = _load("trlx.pipeline.offline_pipeline", "trlx/pipeline/offline_pipeline.py")
    orch = _shell("trlx.orchestrator")
    orch.Orchestrator = type("Orchestrator", (), {})
    orch.register_orchestrator = lambda cls: cls
    return _load("trlx.orchestrator.offline_orchestrator", "trlx/orchestrator/offline_orchestrator.py"), pipe


class CharTokenizer:
    """One token per character (ids 1..95 for the printable ASCII range)."""

    def __call__(self, s):
        return types.SimpleNamespace(input_ids=[ord(c) - 31 for c in s])

    def decode(self, ids):
        return "".join(chr(int(i) + 31) for i in ids)


class Model:
    def __init__(self, tokenizer):
        self.tokenizer = tokenizer
        self.store = None

    def tokenize(self, samples):
        return [self.tokenizer(s).input_ids for s in samples]


def draw_rewards(n, g):
    return (3 * torch.randn(n, generator=g) + 1).tolist()


def record(out, case, orchestrator_cls, model, split_token, samples, rewards, index_lists):
    orch = orchestrator_cls(model, split_token=split_token)
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # std() of one element (case c)
        orch.make_experience(samples, rewards)
    store = model.store
    out[f"{case}/raw_rewards"] = np.asarray(rewards, dtype=np.float32)
    for f in FIELDS:
        ts = getattr(store, f)
        out[f"{case}/{f}"] = torch.cat([t.reshape(-1) for t in ts]).numpy().copy()
        out[f"{case}/{f}_len"] = np.array([t.shape[0] for t in ts], dtype=np.int64)
    out[f"{case}/prompt_lens"] = np.array([int(s[0]) + 1 for s in store.states_ixs], dtype=np.int64)
    collate_fn = store.create_loader(4).collate_fn  # the loader's own order is shuffled; not recorded
    for k, ix in enumerate(index_lists):
        batch = collate_fn([store[i] for i in ix])
        out[f"{case}/batch{k}/ix"] = np.array(ix, dtype=np.int64)
        for f in FIELDS:
            out[f"{case}/batch{k}/{f}"] = getattr(batch, f).numpy().copy()
    out[f"{case}/n_batches"] = np.array(len(index_lists))
    # the fp32 returns against the fp64 evaluation of the same formula
    got = torch.stack([r[-1] for r in store.rewards]).double()
    r64 = torch.tensor(rewards, dtype=torch.float).double()
    if len(rewards) > 1:
        want = (r64 - r64.mean()) / (r64.std() + 1e-30)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    else:
        assert bool(torch.isnan(got).all())
    return store


def main():
    orch_mod, _ = load_offline()
    cls = orch_mod.OfflineOrchestrator
    out = {}

    # a: token lists, prompt length 1
    g = gen(900)
    lens = [2, 3, 63, 64, 65, 129, 5, 17, 31, 100, 8, 2]
    samples = [torch.randint(1, 50, (n,), generator=g).tolist() for n in lens]
    ixs = [[0, 3, 3, 1],               # a repeat
           [11, 9, 7, 5, 2],           # descending
           [5],                        # a single row (the longest)
           [1, 5, 0],                  # the widest row is not first
           list(range(12)),            # every sample, the last one included
           [11, 0]]                    # the two shortest rows
    record(out, "a", cls, Model(None), None, samples, draw_rewards(len(lens), g), ixs)

    # b: strings through a character tokenizer, split on SPLIT
    g = gen(901)
    strings = []
    for pl, cl in [(1, 1), (4, 9), (9, 2), (2, 20), (6, 6), (3, 1)]:
        letters = torch.randint(97, 123, (pl + cl,), generator=g).tolist()
        strings.append("".join(map(chr, letters[:pl])) + SPLIT + "".join(map(chr, letters[pl:])))
    store = record(out, "b", cls, Model(CharTokenizer()), SPLIT, strings, draw_rewards(len(strings), g),
                   [[0, 1, 2, 3, 4, 5], [5, 5, 0], [2], [4, 3, 1], [5, 3, 2, 0]])
    out["b/strings"] = np.array(strings)
    out["b/split_token"] = np.array(SPLIT)
    assert [int(p) for p in out["b/prompt_lens"]] == [s.index(SPLIT) + len(SPLIT) for s in strings]
    assert len(set(out["b/prompt_lens"].tolist())) > 1
    del store

    # c: one sample
    g = gen(902)
    record(out, "c", cls, Model(None), None, [torch.randint(1, 50, (7,), generator=g).tolist()], draw_rewards(1, g),
           [[0], [0, 0]])
    assert bool(np.isnan(out["c/rewards"][-1])) and not np.isnan(out["c/rewards"][:-1]).any()

    path = os.path.join(OUT, "ilql_store.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
