"""The torch restatement of the reference's offline data path (tests/ilql_store_checks.py)
against the fixture recorded from the reference itself (tests/golden/ilql_store.npz, made by
tests/golden/make_golden_ilql_store.py): every recorded list and batch bit for bit, in dtype and
shape too.  The returns are the one exception — (r - mean) / (std + 1e-30) in fp32 depends on
the summation order of mean() and std() — and are held at rtol 1e-5 / atol 1e-6, the bar the
fixture's generator asserts between the reference's fp32 returns and their fp64 evaluation.
No GPU."""
import numpy as np
import pytest
import torch

import ilql_store_checks as C

CASES = ("a", "b", "c")
RET_TOL = dict(rtol=1e-5, atol=1e-6)


def fixture_lists(z, case):
    return {f: C.split_flat(z[f"{case}/{f}"], z[f"{case}/{f}_len"]) for f in C.FIELDS}


def test_fixture_covers_the_required_cases(golden):
    z = golden("ilql_store")
    lens = z["a/input_ids_len"].tolist()
    assert {2, 3, 63, 64, 65, 129} <= set(lens) and 10 <= len(lens) <= 14
    assert set(z["a/prompt_lens"].tolist()) == {1}
    assert len(set(z["b/prompt_lens"].tolist())) > 1
    assert len(z["c/input_ids_len"]) == 1 and bool(np.isnan(z["c/rewards"][-1]))
    ixs = [z[f"a/batch{k}/ix"].tolist() for k in range(int(z["a/n_batches"]))]
    assert any(len(set(ix)) < len(ix) for ix in ixs), "a repeat"
    assert any(len(ix) > 1 and ix == sorted(ix, reverse=True) for ix in ixs), "a descending order"
    assert any(len(ix) == 1 for ix in ixs), "a single row"
    assert any(len(ix) > 1 and int(np.argmax([lens[i] for i in ix])) != 0 for ix in ixs), "widest row not first"
    assert any(len(lens) - 1 in ix for ix in ixs), "the last sample"
    for case in CASES:  # the three offset families
        for a, b in (("attention_mask", "input_ids"), ("dones", "states_ixs"), ("rewards", "actions_ixs")):
            assert z[f"{case}/{a}_len"].tolist() == z[f"{case}/{b}_len"].tolist()


@pytest.mark.parametrize("case", CASES)
def test_make_experience_restatement_equals_the_reference(golden, case):
    z = golden("ilql_store")
    want = fixture_lists(z, case)
    p = z[f"{case}/prompt_lens"]
    got = C.make_experience(want["input_ids"], torch.from_numpy(z[f"{case}/raw_rewards"]),
                            None if case != "b" else p)
    for f in C.FIELDS:
        assert len(got[f]) == len(want[f])
        for g, w in zip(got[f], want[f]):
            assert g.dtype == w.dtype and g.shape == w.shape, f
            if f == "rewards":
                torch.testing.assert_close(g, w, equal_nan=True, **RET_TOL)
                assert torch.equal(torch.isnan(g), torch.isnan(w))
                assert torch.equal(g[:-1], w[:-1])  # the zeros are exact
            else:
                assert torch.equal(g, w), f


@pytest.mark.parametrize("case", CASES)
def test_returns_fp64_is_the_bar(golden, case):
    """The helper the GPU test measures against: the reference's fp32 returns lie within the
    tolerance of it (NaN for one sample)."""
    z = golden("ilql_store")
    ref = torch.stack([r[-1] for r in fixture_lists(z, case)["rewards"]])
    want = C.returns_fp64(torch.from_numpy(z[f"{case}/raw_rewards"]))
    torch.testing.assert_close(ref.double(), want, equal_nan=True, **RET_TOL)
    assert bool(torch.isnan(want).all()) == (case == "c")


@pytest.mark.parametrize("case", CASES)
def test_collate_restatement_equals_the_reference(golden, case):
    z = golden("ilql_store")
    lists = fixture_lists(z, case)
    nb = int(z[f"{case}/n_batches"])
    assert nb >= 2
    for k in range(nb):
        got = C.collate(lists, z[f"{case}/batch{k}/ix"].tolist())
        for f in C.FIELDS:
            w = torch.from_numpy(z[f"{case}/batch{k}/{f}"])
            g = got[f]
            assert g.dtype == w.dtype and g.shape == w.shape, (k, f)
            if f == "rewards":  # NaN (case c) compares unequal to itself: compare the bits
                assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (k, f)
            else:
                assert torch.equal(g, w), (k, f)
