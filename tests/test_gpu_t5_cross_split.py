"""The split decode cross-attention on the GPU (trlx_t5_decode_attn_split: k_t5_decode_attn_split_part,
k_t5_decode_attn_split_merge; t5_decode_cross_attention_split).

Two anchors are equality of the raw bits with the grouped call: X = 1, and any X under a key mask
that leaves live keys in one range only (the chains of that range and the merge then degenerate to
the unsplit kernel's, so an indexing error in a range shows as a bit difference).  For X > 1 with
keys in several ranges the merge order differs from the unsplit kernel's, and the yardstick is the
float64 oracle with torch's eager route on the device, under t5_decode_attn_checks' rule, unchanged:
bf16 e_kernel <= e_torch + one bf16 ulp of max|oracle|, fp32 e_kernel <= 4 * e_torch.  Everything
else is equality of bits between two split calls.  Rows the call must not read hold NaN.

TRLX_T5_CROSS_SPLIT_PARITY_OUT=<file>: the worst e_kernel / bound per dtype is written there
(profiles/t5_cross_split_parity.json is such a run)."""
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
GEOMETRIES = [(dt, d) for dt in A.DTYPES for d in A.D_KVS]
GEOMETRY_IDS = [f"{A.dtype_name(dt)}-d{d}" for dt, d in GEOMETRIES]
CASES = [(dt, d, X) for dt, d in GEOMETRIES for X in S.XS]
CASE_IDS = [f"{g}-X{X}" for g in GEOMETRY_IDS for X in S.XS]
grouped = P.t5_decode_cross_attention_grouped
split = P.t5_decode_cross_attention_split
_WORST = {}


def dev(x):
    return None if x is None else x.to(DEV)


def case(dtype, d, Sn, kind, Gn):
    c = S.group_case(dtype, d, Sn, kind, Gn)
    return dev(c["q"]), dev(c["K"]), dev(c["V"]), dev(c["mask"]), c


def nan_rows(x, rows):
    x = x.clone()
    x[rows] = float("nan")
    return x


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_T5_CROSS_SPLIT_PARITY_OUT")
    if path and _WORST:
        with open(path, "w") as f:
            json.dump({"rule": "bf16: e_kernel <= e_torch + one bf16 ulp of max|oracle|; fp32: e_kernel <= 4 * e_torch; "
                               "e = max abs error against the float64 oracle, e_torch = torch's eager route in the "
                               "input dtype on the device",
                       "cases": "dtype x d_kv 64, 128 x X 1, 2, 3, 4, 8 x G 1, 3, 5 x S 1, 9, 33, 200, 257 x masks none, "
                                "right, left, holes; P 3, nH 5",
                       "worst_e_kernel_over_bound": _WORST}, f, indent=1)
            f.write("\n")


# ------------------------------------------------------------------ 1. anchor: X = 1
@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_one_split_has_the_bits_of_the_grouped_call(dtype, d):
    for Sn in S.SS:
        for kind in A.MASKS:
            for Gn in S.GS:
                q, K, V, mask, _ = case(dtype, d, Sn, kind, Gn)
                got = split(q, K, V, mask, groups=Gn, splits=1)
                assert got.dtype == dtype and tuple(got.shape) == (S.P * Gn, S.NH * d) and got.is_contiguous()
                assert C.same(got, grouped(q, K, V, mask)), (Sn, kind, Gn)


# ------------------------------------------------------------------ 2. anchor: one range live
@pytest.mark.parametrize("dtype,d,X", CASES, ids=CASE_IDS)
def test_with_one_range_live_the_bits_are_the_grouped_calls(dtype, d, X):
    for Sn in S.SS:
        g = P.t5_decode_cross_attention_split_geometry(dtype, d, Sn, X)
        assert {k: g[k] for k in ("NG", "C", "ranges")} == S.geometry(dtype, d, Sn, X)
        for Gn in S.GS:
            q, K, V, _, _ = case(dtype, d, Sn, "none", Gn)
            for x in range(g["ranges"]):
                mask = dev(S.range_mask(Sn, g["C"], x))
                assert C.same(split(q, K, V, mask, groups=Gn, splits=X), grouped(q, K, V, mask)), (Sn, Gn, x, g)


# ------------------------------------------------------------------ 3. accuracy, every mask
@pytest.mark.parametrize("dtype,d,X", CASES, ids=CASE_IDS)
def test_the_error_against_the_float64_oracle_is_within_torchs_own(dtype, d, X):
    """max|kernel - oracle| <= bound(max|eager - oracle|): t5_decode_attn_checks' rule, unchanged.  The
    kernel sees K / V with NaN in the masked rows."""
    name = A.dtype_name(dtype)
    for Sn in S.SS:
        for kind in A.MASKS:
            for Gn in S.GS:
                want, e_t = S.reference(dtype, d, Sn, kind, Gn, "cuda:0")
                q, _, _, mask, c = case(dtype, d, Sn, kind, Gn)
                got = split(q, dev(A.poison(c["K"], c["mask"])), dev(A.poison(c["V"], c["mask"])), mask, groups=Gn, splits=X)
                e_k = A.max_err(got, want)
                lim = A.bound(dtype, e_t, want)
                fig = dict(dtype=name, d_kv=d, X=X, S=Sn, mask=kind, G=Gn, e_torch=e_t, e_kernel=e_k, bound=lim)
                print(fig)
                ratio = 0.0 if e_k == 0.0 else (e_k / lim if lim > 0 else float("inf"))
                if ratio >= _WORST.get(name, {}).get("e_kernel_over_bound", -1.0):
                    _WORST[name] = dict(fig, e_kernel_over_bound=ratio)
                assert torch.isfinite(got.float()).all() and e_k <= lim, fig


# ------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("dtype,d,X", CASES, ids=CASE_IDS)
def test_the_result_depends_on_the_splits_alone(dtype, d, X):
    """Not on the layout of K / V, the query tile, the call before or the other prompts."""
    inner = S.NH * d
    try:
        for Sn in (33, 200, 257):
            for Gn in S.GS:
                q, K, V, mask, c = case(dtype, d, Sn, "holes", Gn)
                want = split(q, K, V, mask, groups=Gn, splits=X)
                assert C.same(split(q, K, V, mask, groups=Gn, splits=X), want), (Sn, Gn, "two consecutive calls")
                # the projection output [P, S, nH * d], read in place
                k3 = dev(c["K"].permute(0, 2, 1, 3).reshape(S.P, Sn, inner).contiguous())
                v3 = dev(c["V"].permute(0, 2, 1, 3).reshape(S.P, Sn, inner).contiguous())
                assert k3.stride() == (Sn * inner, inner, 1)
                assert C.same(split(q, k3, v3, mask, n_heads=S.NH, groups=Gn, splits=X), want), (Sn, Gn, "layout")
                for tile in (1, 2, 4, 8):
                    P.t5_decode.t5_decode_cross_attention_group_tile(tile)
                    assert C.same(split(q, K, V, mask, groups=Gn, splits=X), want), (Sn, Gn, "tile", tile)
                P.t5_decode.t5_decode_cross_attention_group_tile(0)
                alone = split(q[:Gn], K[:1], V[:1], mask[:1], groups=Gn, splits=X)
                assert C.same(alone, want[:Gn]), (Sn, Gn, "prompt 0 alone")
    finally:
        P.t5_decode.t5_decode_cross_attention_group_tile(0)


# ------------------------------------------------------------------ 5. masked keys are not read
@pytest.mark.parametrize("dtype,d,X", CASES, ids=CASE_IDS)
def test_masked_keys_are_not_read_and_a_fully_masked_prompt_gives_zeros(dtype, d, X):
    for Sn in S.SS:
        for kind in ("right", "left", "holes"):
            for Gn in S.GS:
                q, K, V, mask, c = case(dtype, d, Sn, kind, Gn)
                want = split(q, K, V, mask, groups=Gn, splits=X)
                assert torch.isfinite(want.float()).all()
                got = split(q, dev(A.poison(c["K"], c["mask"])), dev(A.poison(c["V"], c["mask"])), mask, groups=Gn, splits=X)
                assert C.same(got, want), (Sn, kind, Gn)
                m0 = c["mask"].clone()
                m0[1] = 0                                             # prompt 1 has no live key
                got = split(q, dev(A.poison(c["K"], m0)), dev(A.poison(c["V"], m0)), dev(m0), groups=Gn, splits=X)
                assert not got[Gn:2 * Gn].any() and not torch.isnan(got.float()).any(), (Sn, kind, Gn)
                assert C.same(got[:Gn], want[:Gn]) and C.same(got[2 * Gn:], want[2 * Gn:]), (Sn, kind, Gn)


# ------------------------------------------------------------------ 6. live
@pytest.mark.parametrize("dtype,d,X", CASES, ids=CASE_IDS)
def test_dead_rows_get_zeros_and_nothing_of_them_is_read_not_even_their_states(dtype, d, X):
    for Sn in (1, 33, 257):
        for Gn in S.GS:
            q, K, V, mask, c = case(dtype, d, Sn, "holes", Gn)
            Kp, Vp = dev(A.poison(c["K"], c["mask"])), dev(A.poison(c["V"], c["mask"]))
            want = split(q, K, V, mask, groups=Gn, splits=X)
            need = P.t5_decode.t5_decode_cross_attention_split_workspace_bytes(S.P * Gn, S.NH, d, X)
            for name, pattern in S.live_sets(Gn).items():
                live = dev(pattern)
                on = live != 0
                dead_prompts = ~on.view(S.P, Gn).any(dim=1)
                # a workspace full of NaN: a dead tile writes no state and the merge must not read one
                ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
                got = split(nan_rows(q, ~on), nan_rows(Kp, dead_prompts), nan_rows(Vp, dead_prompts), mask, live=live,
                            groups=Gn, splits=X, workspace=ws)
                assert not torch.isnan(got.float()).any(), (Sn, Gn, name)
                assert C.same(got[on], want[on]), (Sn, Gn, name, "live rows")
                assert C.same(got[~on], torch.zeros_like(got[~on])), (Sn, Gn, name, "dead rows")
                assert live.tolist() == pattern.tolist()
                if name == "all_dead":                                # q, K and V all NaN, every prompt dead
                    nan = float("nan")
                    got = split(torch.full_like(q, nan), torch.full_like(K, nan), torch.full_like(V, nan), mask, live=live,
                                groups=Gn, splits=X, workspace=ws)
                    assert C.same(got, torch.zeros_like(got)), (Sn, Gn, name)


# ------------------------------------------------------------------ 7. nothing written out of bounds
@pytest.mark.parametrize("dtype,d,X", CASES, ids=CASE_IDS)
def test_nothing_is_written_before_or_after_the_workspace(dtype, d, X):
    Sn, Gn = 257, 5
    q, K, V, mask, _ = case(dtype, d, Sn, "left", Gn)
    need = P.t5_decode.t5_decode_cross_attention_split_workspace_bytes(S.P * Gn, S.NH, d, X) // 4
    for live in (None, dev(S.live_sets(Gn)["alternating"])):
        whole = torch.full((need + 2 * 1024,), C.GUARD, dtype=torch.float32, device=DEV)
        got = split(q, K, V, mask, live=live, groups=Gn, splits=X, workspace=whole[1024:1024 + need])
        assert C.same(got, split(q, K, V, mask, live=live, groups=Gn, splits=X))
        edge = torch.full((1024,), C.GUARD, dtype=torch.float32, device=DEV)
        assert C.same(whole[:1024], edge) and C.same(whole[1024 + need:], edge)
    with pytest.raises(ValueError, match="workspace"):
        split(q, K, V, mask, groups=Gn, splits=X, workspace=whole[:need - 1])
    with pytest.raises(ValueError, match="workspace"):
        split(q, K, V, mask, groups=Gn, splits=X, workspace=whole[1:1 + need])      # 4 bytes off the alignment


# ------------------------------------------------------------------ 8. splits=None takes the plan
def test_the_default_takes_the_plan(monkeypatch):
    dtype, d, Gn, Sn = torch.bfloat16, 64, 3, 1100                    # 15 workgroups, 35 keys a group: the plan splits
    X = P.t5_decode_cross_attention_split_plan(dtype, S.P, Gn, S.NH, d, Sn)
    assert 1 < X <= S.CAP
    q, K, V, mask, _ = case(dtype, d, Sn, "holes", Gn)
    seen = []
    real = P._lib.call
    monkeypatch.setattr(P._lib, "call", lambda name, *a: (seen.append((name, a[1])), real(name, *a))[1])
    got = split(q, K, V, mask, groups=Gn)
    assert seen[-1] == ("trlx_t5_decode_attn_split", X)
    assert C.same(got, split(q, K, V, mask, groups=Gn, splits=X))
    want, e_t = S.reference(dtype, d, Sn, "holes", Gn, "cuda:0")
    assert A.max_err(got, want) <= A.bound(dtype, e_t, want)
    assert P.t5_decode_cross_attention_split_plan(dtype, S.P, Gn, S.NH, d, 9) == 1
    assert C.same(split(*case(dtype, d, 9, "holes", Gn)[:4], groups=Gn), grouped(*case(dtype, d, 9, "holes", Gn)[:4]))


# ------------------------------------------------------------------ 9. capture
@pytest.mark.parametrize("X", (2, 8))
def test_one_captured_call_replays_on_changed_q(X):
    dtype, d, Gn, Sn = torch.bfloat16, 64, 5, 257
    q, K, V, mask, _ = case(dtype, d, Sn, "holes", Gn)
    qs = [dev(S.group_case(dtype, d, Sn, kind, Gn)["q"]) for kind in ("none", "right", "left")]
    q_in = q.clone()
    split(q_in, K, V, mask, groups=Gn, splits=X)                      # warm up outside the capture: the workspace exists
    torch.cuda.synchronize()
    held = {k: w.data_ptr() for k, w in P.t5_decode._SPLIT_WORKSPACES.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # one stream, two launches in order
        out = split(q_in, K, V, mask, groups=Gn, splits=X)
    for qn in qs:
        q_in.copy_(qn)
        graph.replay()
        torch.cuda.synchronize()
        assert {k: w.data_ptr() for k, w in P.t5_decode._SPLIT_WORKSPACES.items()} == held
        got = out.clone()
        assert C.same(got, split(qn, K, V, mask, groups=Gn, splits=X))
    assert {k: w.data_ptr() for k, w in P.t5_decode._SPLIT_WORKSPACES.items()} == held
