"""Torch restatement of the two reference functions the ILQL store replaces, on host tensors:

  make_experience  OfflineOrchestrator.make_experience (offline_orchestrator.py:26-70) for
                   already tokenised samples: the six per-sample lists.
  collate          ILQLRolloutStorage.create_loader's collate_fn (offline_pipeline.py:88-108):
                   six pad_sequence calls over the chosen elements.

tests/test_ilql_store_cpu.py pins both to the fixture recorded from the reference itself
(tests/golden/ilql_store.npz); the GPU tests then use them at other shapes.
"""
import torch
from torch.nn.utils.rnn import pad_sequence

FIELDS = ("input_ids", "attention_mask", "rewards", "states_ixs", "actions_ixs", "dones")
FAMILY = dict(input_ids="L", attention_mask="L", rewards="A", states_ixs="S", actions_ixs="A", dones="S")


def make_experience(input_ids, rewards, prompt_lens=None):
    """{field: list of 1-D tensors}; prompt_lens None = 1 (the bos-token case)."""
    input_ids = [torch.as_tensor(t) for t in input_ids]
    n = len(input_ids)
    prompt_lens = [1] * n if prompt_lens is None else [int(p) for p in prompt_lens]
    actions_ixs = [torch.arange(p - 1, len(t) - 1) for p, t in zip(prompt_lens, input_ids)]
    states_ixs = [torch.arange(p - 1, len(t)) for p, t in zip(prompt_lens, input_ids)]
    dones = []
    for s in states_ixs:
        d = torch.ones_like(s)
        d[-1] = 0
        dones.append(d)
    returns = torch.as_tensor(rewards, dtype=torch.float)
    returns = (returns - returns.mean()) / (returns.std() + 1e-30)
    rs = [torch.zeros(a.shape[0]) for a in actions_ixs]
    for r, G in zip(rs, returns):
        r[-1] = G
    attention_mask = [torch.ones(t.shape[0], dtype=torch.int64) for t in input_ids]
    return dict(input_ids=input_ids, attention_mask=attention_mask, rewards=rs, states_ixs=states_ixs,
                actions_ixs=actions_ixs, dones=dones)


def returns_fp64(rewards):
    """The same formula evaluated in fp64 on the fp32 rewards (the bar the fp32 results are held to)."""
    r = torch.as_tensor(rewards, dtype=torch.float).double()
    return (r - r.mean()) / (r.std() + 1e-30)


def collate(lists, ix):
    """{field: [len(ix), W] tensor} of the elements `ix` (any order, repeats allowed)."""
    pad = dict(rewards=0.0)
    return {f: pad_sequence([lists[f][i] for i in ix], batch_first=True, padding_value=pad.get(f, 0)) for f in FIELDS}


def split_flat(flat, lens):
    """A flat array and its per-sample lengths back to the list of 1-D tensors."""
    return list(torch.split(torch.as_tensor(flat), [int(v) for v in lens]))
