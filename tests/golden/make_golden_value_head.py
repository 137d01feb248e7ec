"""Generate tests/golden/value_head.npz from the REFERENCE's make_head(n_embd, 1)
(trlx/model/nn/ppo_models.py:216-222): the bf16 value head's seeded weights, a seeded input, its
CPU output and the gradients its own bf16 autograd gives for a seeded dv.  Data only — bf16
tensors as raw uint16 bits, no code.

Like make_golden.py (whose reference loader it uses) this runs only where the reference
checkout is present; the fixture it writes is plain data.

Run:  python tests/golden/make_golden_value_head.py
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

from make_golden import gen, load_reference, store  # noqa: E402

H, N = 64, 20


def main():
    _, ppo_models, _, _ = load_reference()
    torch.manual_seed(1234)
    head = ppo_models.make_head(H, 1)
    sd = head.state_dict()
    g = gen(77)
    h = torch.randn(N, H, generator=g).to(torch.bfloat16).requires_grad_(True)
    dv = torch.randn(N, 1, generator=g).to(torch.bfloat16)
    out = head(h)
    out.backward(dv)
    res = {"H": np.array(H), "N": np.array(N), "names": np.array(list(sd.keys())), "h": store(h), "dv": store(dv),
           "out": store(out), "dh": store(h.grad)}
    for k, v in sd.items():
        assert v.dtype == torch.bfloat16
        res["sd/" + k] = store(v)
    for k, p in head.named_parameters():
        res["grad/" + k] = store(p.grad)
    path = os.path.join(OUT, "value_head.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
