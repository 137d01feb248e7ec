"""Generate tests/golden/ilql_heads_keys.npz from the REFERENCE's ILQLHeads
(trlx/model/nn/ilql_models.py:119-136): the state_dict's parameter names and shapes, for one
and two Q heads.  Names and shapes only — no weights, no code.

Like make_golden.py (whose reference loader it uses) this runs only where the reference
checkout is present; the fixture it writes is plain data.

Run:  python tests/golden/make_golden_ilql_heads.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

from make_golden import load_reference  # noqa: E402

HIDDEN, VOCAB = 16, 37


def main():
    _, _, ilql_models, _ = load_reference()
    out = {"hidden_size": np.array(HIDDEN), "vocab_size": np.array(VOCAB)}
    for two_qs in (False, True):
        cfg = ilql_models.ILQLConfig(name="ilqlconfig", tau=0.7, gamma=0.99, cql_scale=0.1, awac_scale=1,
                                     alpha=0.001, steps_for_target_q_sync=5, betas=[4], two_qs=two_qs)
        sd = ilql_models.ILQLHeads(cfg, HIDDEN, VOCAB).state_dict()
        k = f"two_qs{int(two_qs)}"
        out[f"{k}/names"] = np.array(list(sd.keys()))
        out[f"{k}/ndim"] = np.array([v.dim() for v in sd.values()], dtype=np.int64)
        shapes = np.zeros((len(sd), 2), dtype=np.int64)
        for i, v in enumerate(sd.values()):
            shapes[i, :v.dim()] = list(v.shape)
        out[f"{k}/shapes"] = shapes
    path = os.path.join(OUT, "ilql_heads_keys.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
