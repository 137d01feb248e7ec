"""The shared cases of the split decode cross-attention (trlx_t5_decode_attn_split,
csrc/t5_decode_attn_split.hip; tests/test_t5_cross_split_cpu.py, tests/test_gpu_t5_cross_split.py).

A case is group_case of t5_cross_group_checks: P = 3 prompts, nH = 5 heads, K / V [P, nH, S, d], a
mask [P, S] per prompt and a q of P * G rows.

  XS            the splits: 1 (the grouped call), 2, 3 (ranges of unequal fill), 4, 8 (the cap)
  GS            one query a prompt (the plain cross-attention), a remainder tile (3), a whole tile
                and a remainder (5)
  SS            1 (seven of eight ranges empty at X 8), 9 and 33 (ranges shorter than the groups of
                a workgroup, so most ranges are empty), 200 and 257 (both sides of the range edges
                and of the multiples of NG 8 / 16 / 32 at every X)
  geometry      the reference geometry in Python: NG, C = ceil(S / X) rounded up to NG, the ranges
  range_mask    a key mask that keeps the keys of one range only
  reference     the float64 oracle and the error of torch's eager route on `device` for a case,
                computed once per (dtype, d_kv, S, kind, G) and shared by every X

Test infrastructure only."""
import functools

import torch

from t5_decode_attn_checks import cross_case, make_mask, oracle_cross, eager_cross, bound, poison  # noqa: F401
from t5_decode_attn_checks import MASKS, max_err
from t5_cross_group_checks import group_case, expand, live_sets  # noqa: F401
from t5_cross_group_checks import P, NH, groups

XS = (1, 2, 3, 4, 8)
GS = (1, 3, 5)
SS = (1, 9, 33, 200, 257)
CAP = 8


def geometry(dtype, d_kv, S, X):
    """dict(NG, C, ranges) as the header states them."""
    ng = groups(dtype, d_kv)
    c = -(-S // X)
    c = -(-c // ng) * ng
    return dict(NG=ng, C=c, ranges=-(-S // c))


def range_mask(S, C, x):
    """int64 [P, S]: keys [x * C, min(S, (x + 1) * C)) live, every other key masked."""
    m = torch.zeros(P, S, dtype=torch.int64)
    m[:, x * C:min(S, (x + 1) * C)] = 1
    return m


@functools.lru_cache(maxsize=None)
def reference(dtype, d_kv, S, kind, G, device):
    """(want float64 [P*G, nH*d] on the CPU, e_torch) of group_case(dtype, d_kv, S, kind, G): the
    oracle reads K / V with NaN in the masked rows, torch's eager route the clean ones on `device`."""
    c = group_case(dtype, d_kv, S, kind, G)
    q3 = c["q"].reshape(P * G, NH, d_kv)
    mx = expand(c["mask"], G)
    want = oracle_cross(q3, expand(poison(c["K"], c["mask"]), G), expand(poison(c["V"], c["mask"]), G), mx)
    dev = torch.device(device)
    eager = eager_cross(q3.to(dev), expand(c["K"], G).to(dev), expand(c["V"], G).to(dev), None if mx is None else mx.to(dev))
    return want, max_err(eager, want)


assert MASKS == ("none", "right", "left", "holes")
