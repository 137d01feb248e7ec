"""The grouped decode cross-attention on MFMA at d_kv 256 on the GPU (trlx_t5_decode_attn_group_d256:
k_t5_decode_attn_group_d256, k_t5_decode_attn_group_d256_merge; t5_decode_cross_attention_grouped_mma_d256).

The yardstick is the float64 oracle with torch's eager bf16 route on the device, under the rule of
the 64 / 128 kernel (P is rounded to bf16 un-normalised): max|kernel - oracle| <= 2 * e_torch + one
bf16 ulp of max|oracle|.  Everything else is equality of bits between two calls of the route.  Rows
the call must not read hold NaN.  TRLX_T5_CROSS_GROUP_D256_PARITY_OUT=<file>: the worst e_kernel /
bound is written there (profiles/t5_cross_group_d256_parity.json)."""
import json
import os

import pytest
import torch

import trlx_t5_amd as P
import t5_cross_split_checks as S
import t5_decode_attn_checks as A
import t5_rollout_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF, D = torch.bfloat16, 256
d256 = P.t5_decode_cross_attention_grouped_mma_d256
SS = (1, 31, 32, 33, 127, 128, 129, 200)    # both sides of a 32-key block and of one round of the 4 waves
GS = (1, 7, 16, 17, 33)                     # below a tile, a full tile, a remainder of one row after one and two tiles
XS = (1, 2, 3, 8)                           # ranges of unequal fill; at S 1 and 33 fewer ranges than splits
_WORST = {}


def dev(x):
    return None if x is None else x.to(DEV)


def case(Sn, kind, Gn):
    """q, K, V (NaN in the masked rows) and the mask on the device."""
    c = S.group_case(BF, D, Sn, kind, Gn)
    return dev(c["q"]), dev(S.poison(c["K"], c["mask"])), dev(S.poison(c["V"], c["mask"])), dev(c["mask"])


def nan_rows(x, rows):
    x = x.clone()
    x[rows] = float("nan")
    return x


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_CROSS_GROUP_D256_PARITY_OUT")
    if path and _WORST:
        with open(path, "w") as f:
            json.dump({"rule": "e_kernel <= 2 * e_torch + one bf16 ulp of max|oracle|; e = max abs error against the "
                               "float64 oracle, e_torch = torch's eager bf16 route on the device",
                       "cases": f"bf16 d_kv 256 x S {SS} x G {GS} x splits {XS} x masks {A.MASKS}; P 3, nH 5; K / V hold "
                                "NaN in the masked rows", "worst_e_kernel_over_bound": _WORST}, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("Sn,Gn,X", [(Sn, Gn, X) for Sn in SS for Gn in GS for X in XS])
def test_the_error_against_the_float64_oracle_is_within_twice_torchs_own(Sn, Gn, X):
    for kind in A.MASKS:
        want, e_t = S.reference(BF, D, Sn, kind, Gn, "cuda:0")
        q, K, V, mask = case(Sn, kind, Gn)
        got = d256(q, K, V, mask, splits=X)
        assert got.dtype == BF and tuple(got.shape) == (S.P * Gn, S.NH * D) and got.is_contiguous()
        e_k, lim = A.max_err(got, want), 2.0 * e_t + A.bf16_ulp(float(want.abs().max()))
        print(dict(S=Sn, G=Gn, splits=X, mask=kind, e_torch=e_t, e_kernel=e_k, bound=lim))
        if e_k / lim >= _WORST.get("e_kernel_over_bound", -1.0):
            _WORST.update(S=Sn, G=Gn, splits=X, mask=kind, e_torch=e_t, e_kernel=e_k, bound=lim, e_kernel_over_bound=e_k / lim)
        assert torch.isfinite(got.float()).all() and e_k <= lim, (kind, e_k, lim)


@pytest.mark.parametrize("X", (1, 3))
def test_a_rows_bits_are_its_own(X):
    """Not the group size's, the tile place's, the K / V layout's, the q stride's or the workspace's."""
    Gn, Sn, inner = 17, 200, S.NH * D
    q, K, V, mask = case(Sn, "holes", Gn)
    want = d256(q, K, V, mask, splits=X)
    assert C.same(d256(q, K, V, mask, splits=X), want)
    last = d256(q[Gn - 1::Gn].contiguous(), K, V, mask, splits=X)     # the remainder tile's one row, as a G 1 call
    assert C.same(last, want[Gn - 1::Gn])
    k3, v3 = (x.permute(0, 2, 1, 3).reshape(S.P, Sn, inner).contiguous() for x in (K, V))
    assert C.same(d256(q, k3, v3, mask, n_heads=S.NH, splits=X), want)   # the projection output, read in place
    wide = torch.full((S.P * Gn, inner + 64), float("nan"), dtype=BF, device=DEV)
    wide[:, :inner] = q
    assert wide[:, :inner].stride(0) == inner + 64 and C.same(d256(wide[:, :inner], K, V, mask, splits=X), want)
    need = P.t5_decode_cross_attention_grouped_mma_d256_workspace_bytes(S.P * Gn, S.NH, Sn, X)
    assert (need == 0) == (X == 1)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device=DEV)   # every float in it a NaN
    assert C.same(d256(q, K, V, mask, splits=X, workspace=ws), want)


@pytest.mark.parametrize("Gn,X", [(Gn, X) for Gn in (7, 17) for X in (1, 3)])
def test_dead_rows_get_zeros_and_live_rows_keep_their_bits(Gn, X):
    q, K, V, mask = case(200, "holes", Gn)
    want = d256(q, K, V, mask, splits=X)
    for name, pattern in S.live_sets(Gn).items():
        live = dev(pattern)
        on = live != 0
        dead_prompts = ~on.view(S.P, Gn).any(dim=1)                   # none of their K / V may be read
        got = d256(nan_rows(q, ~on), nan_rows(K, dead_prompts), nan_rows(V, dead_prompts), mask, live=live, splits=X)
        assert not torch.isnan(got.float()).any(), name
        assert C.same(got[on], want[on]), (name, "live rows")
        assert C.same(got[~on], torch.zeros_like(got[~on])), (name, "dead rows")


@pytest.mark.parametrize("X", (1, 3))
def test_a_fully_masked_prompt_gives_zeros(X):
    Gn = 17
    q, K, V, mask = case(200, "holes", Gn)
    want = d256(q, K, V, mask, splits=X)
    mask = mask.clone()
    mask[1] = 0
    got = d256(q, nan_rows(K, [1]), nan_rows(V, [1]), mask, splits=X)
    assert C.same(got[Gn:2 * Gn], torch.zeros_like(got[Gn:2 * Gn]))
    assert C.same(got[:Gn], want[:Gn]) and C.same(got[2 * Gn:], want[2 * Gn:])


def test_a_captured_call_replays_with_the_eager_bits():
    Gn = 17
    q, K, V, mask = case(200, "holes", Gn)
    live = dev(S.live_sets(Gn)["alternating"])
    want = d256(q, K, V, mask, live=live, splits=3)                   # the eager call allocates the workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = d256(q, K, V, mask, live=live, splits=3)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert C.same(out, want)


def test_the_grouped_mma_call_takes_the_new_kernel_at_the_plans_splits():
    Gn, Sn = 17, 200
    q, K, V, mask = case(Sn, "holes", Gn)
    X = P.t5_decode_cross_attention_grouped_mma_d256_plan(S.P, Gn, S.NH, Sn)
    assert C.same(P.t5_decode_cross_attention_grouped_mma(q, K, V, mask), d256(q, K, V, mask, splits=X))
    assert C.same(d256(q, K, V, mask), d256(q, K, V, mask, splits=X))
