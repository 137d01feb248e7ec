"""GPU tests of the device-resident ILQL rollout store (trlx-t5_amd/ilql_store.py,
csrc/ilql_store.hip): the ragged collate (trlx_ilql_collate), the device half of
make_experience (trlx_ilql_build_fields), the loader and the store's error checks.

References
  tests/golden/ilql_store.npz  recorded from the reference's own make_experience / collate_fn
  ilql_store_checks.py         their torch restatement (pinned to the fixture by
                               test_ilql_store_cpu.py), used at the shapes the fixture lacks

Tolerances
  collate, integer fields   pure data movement and integer arithmetic: torch.equal, dtype and
                            shape included (the rewards are compared by their bits, NaN too).
  returns                   rtol 1e-5 / atol 1e-6, the project's fp32 bar.  The device evaluates
                            (r - mean) / (std + 1e-30) in fp64 and rounds once; the fixture's
                            generator asserts that the reference's fp32 returns lie within the
                            same bar of that fp64 evaluation, for rewards drawn as 3·N(0,1) + 1.
"""
import numpy as np
import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import ilql_store_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RET_TOL = dict(rtol=1e-5, atol=1e-6)
CASES = ("a", "b", "c")
FILL = -7


def fixture_lists(z, case):
    return {f: C.split_flat(z[f"{case}/{f}"], z[f"{case}/{f}_len"]) for f in C.FIELDS}


def same(got, want):
    """Equal in dtype, shape and value; fp32 by its bits (NaN included)."""
    got, want = got.cpu(), want.cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == torch.float32:
        return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    return torch.equal(got, want)


def store_of(lists, **kw):
    return P.ILQLRolloutStorage(*[lists[f] for f in C.FIELDS], device=DEV, **kw)


def collate(store, ix):
    rows = np.asarray(ix, dtype=np.int64)
    batch = store.collate(torch.from_numpy(rows).to(DEV), rows)
    torch.cuda.synchronize()
    return batch


def assert_batch(batch, want):
    assert isinstance(batch, P.ILQLBatch)
    for f in C.FIELDS:
        got = getattr(batch, f)
        assert got.is_cuda and same(got, torch.as_tensor(want[f])), f


@pytest.fixture(scope="module")
def stores(golden):
    """The fixture's three cases through the reference constructor (built once, never modified)."""
    z = golden("ilql_store")
    return {case: store_of(fixture_lists(z, case)) for case in CASES}


# ------------------------------------------------------------------ reference constructor + collate
@pytest.mark.parametrize("case", CASES)
def test_collate_equals_the_reference_batches(golden, stores, case):
    z, store = golden("ilql_store"), stores[case]
    for k in range(int(z[f"{case}/n_batches"])):
        batch = collate(store, z[f"{case}/batch{k}/ix"].tolist())
        assert_batch(batch, {f: z[f"{case}/batch{k}/{f}"] for f in C.FIELDS})


@pytest.mark.parametrize("case", CASES)
def test_getitem_equals_the_input_lists(golden, stores, case):
    lists, store = fixture_lists(golden("ilql_store"), case), stores[case]
    n = len(lists["input_ids"])
    assert len(store) == n
    for i in range(n):
        e = store[i]
        assert isinstance(e, P.ILQLElement)
        for f in C.FIELDS:
            assert getattr(e, f).is_cuda and same(getattr(e, f), lists[f][i]), (i, f)
    assert same(store[-1].input_ids, lists["input_ids"][-1])
    with pytest.raises(IndexError):
        store[n]


# ------------------------------------------------------------------ from_samples
@pytest.mark.parametrize("case", CASES)
def test_from_samples_equals_the_reference(golden, case):
    z = golden("ilql_store")
    want = fixture_lists(z, case)
    raw = torch.from_numpy(z[f"{case}/raw_rewards"])
    store = P.ILQLRolloutStorage.from_samples(want["input_ids"], raw, None if case == "a" else z[f"{case}/prompt_lens"],
                                              device=DEV)
    torch.cuda.synchronize()
    n = len(want["input_ids"])
    assert len(store) == n
    for i in range(n):
        e = store[i]
        for f in C.FIELDS:
            g, w = getattr(e, f).cpu(), want[f][i]
            assert g.dtype == w.dtype and g.shape == w.shape, (i, f)
            if f != "rewards":
                assert torch.equal(g, w), (i, f)
                continue
            assert torch.equal(torch.isnan(g), torch.isnan(w)), i  # case c: NaN exactly where the reference is
            assert torch.equal(g[:-1], w[:-1]), i                  # the zeros are exact
            torch.testing.assert_close(g, w, equal_nan=True, **RET_TOL)
    got = torch.stack([store[i].rewards[-1] for i in range(n)]).cpu().double()
    torch.testing.assert_close(got, C.returns_fp64(raw), equal_nan=True, **RET_TOL)
    # and its batches are the reference's (rewards at the returns' tolerance)
    for k in range(int(z[f"{case}/n_batches"])):
        batch = collate(store, z[f"{case}/batch{k}/ix"].tolist())
        for f in C.FIELDS:
            g, w = getattr(batch, f).cpu(), torch.from_numpy(z[f"{case}/batch{k}/{f}"])
            assert g.dtype == w.dtype and g.shape == w.shape, (k, f)
            if f == "rewards":
                torch.testing.assert_close(g, w, equal_nan=True, **RET_TOL)
            else:
                assert torch.equal(g, w), (k, f)


def test_from_samples_tensor_and_list_prompt_lens():
    g = torch.Generator().manual_seed(5)
    ids = [torch.randint(0, 37, (n,), generator=g) for n in (4, 9, 2, 6, 3)]
    rewards = (3 * torch.randn(5, generator=g) + 1).tolist()
    p = [2, 8, 1, 1, 2]
    want = C.make_experience(ids, rewards, p)
    for pl in (p, torch.tensor(p), np.array(p)):
        store = P.ILQLRolloutStorage.from_samples([t.to(DEV) for t in ids], rewards, pl, device=DEV)
        batch = collate(store, [4, 3, 2, 1, 0])
        ref = C.collate(want, [4, 3, 2, 1, 0])
        for f in C.FIELDS:
            if f == "rewards":
                torch.testing.assert_close(getattr(batch, f).cpu(), ref[f], **RET_TOL)
            else:
                assert same(getattr(batch, f), ref[f]), f


# ------------------------------------------------------------------ direct ABI call
def abi_collate(store, ix, widths, extra_cols=3, extra_rows=2):
    """trlx_ilql_collate into buffers of (n + extra_rows) x (W + extra_cols) filled with FILL."""
    n = len(ix)
    idx = torch.tensor(ix, dtype=torch.int64, device=DEV)
    outs = {}
    for f in C.FIELDS:
        w = widths[C.FAMILY[f]]
        outs[f] = torch.full((n + extra_rows, w + extra_cols), FILL, dtype=store._flat[f].dtype, device=DEV)
    _lib.call("trlx_ilql_collate", *[_lib.ptr(store._flat[f]) for f in C.FIELDS], _lib.ptr(store._off["L"]),
              _lib.ptr(store._off["S"]), _lib.ptr(store._off["A"]), len(store), _lib.ptr(idx), n, widths["L"],
              widths["S"], widths["A"], *[v for f in C.FIELDS for v in (_lib.ptr(outs[f]), outs[f].stride(0))],
              _lib.stream_of(idx))
    torch.cuda.synchronize()
    return {f: t.cpu() for f, t in outs.items()}


def check_window(outs, lists, ix, widths):
    """Inside [n, W]: the sample's first W elements, then zeros; outside: still FILL."""
    n = len(ix)
    for f in C.FIELDS:
        w = widths[C.FAMILY[f]]
        o = outs[f]
        want = torch.zeros((n, w), dtype=o.dtype)
        for j, i in enumerate(ix):
            row = lists[f][i][:w]
            want[j, :row.shape[0]] = row
        assert same(o[:n, :w], want), f
        assert bool((o[:n, w:] == FILL).all()) and bool((o[n:] == FILL).all()), f


@pytest.mark.parametrize("ix", [[5], [0, 5, 2, 11], [11, 3, 3, 4, 1]], ids=["n1", "n4", "n5"])
def test_abi_writes_only_its_window(golden, stores, ix):
    lists, store = fixture_lists(golden("ilql_store"), "a"), stores["a"]
    widths = {k: max(int(lists[f][i].shape[0]) for i in ix) for k, f in
              (("L", "input_ids"), ("S", "states_ixs"), ("A", "actions_ixs"))}
    check_window(abi_collate(store, ix, widths), lists, ix, widths)


def test_abi_truncates_rows_longer_than_the_width(golden, stores):
    lists, store = fixture_lists(golden("ilql_store"), "a"), stores["a"]
    ix = [5, 0, 9, 2, 1]  # lengths 129, 2, 100, 63, 3
    widths = {"L": 66, "S": 64, "A": 7}
    check_window(abi_collate(store, ix, widths), lists, ix, widths)


def test_abi_edges(golden, stores):
    store = stores["a"]
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    outs = [torch.full((2, 4), FILL, dtype=store._flat[f].dtype, device=DEV) for f in C.FIELDS]
    flat = [_lib.ptr(store._flat[f]) for f in C.FIELDS]
    offs = [_lib.ptr(store._off[k]) for k in ("L", "S", "A")]

    def call(n=2, w=(4, 4, 4), ld=4, idx_p=_lib.ptr(idx), flat_p=flat, out0=_lib.ptr(outs[0])):
        ptrs = [out0] + [_lib.ptr(o) for o in outs[1:]]
        _lib.call("trlx_ilql_collate", *flat_p, *offs, len(store), idx_p, n, *w,
                  *[v for p in ptrs for v in (p, ld)], _lib.stream_of(idx))

    call(n=0)  # no launch, nothing written
    torch.cuda.synchronize()
    assert all(bool((o == FILL).all()) for o in outs)
    for bad in (dict(n=-1), dict(w=(-1, 4, 4)), dict(ld=3), dict(idx_p=None), dict(flat_p=[None] + flat[1:]),
                dict(out0=None)):
        with pytest.raises(ValueError):
            call(**bad)
    # a sample number outside the store gives a row of pads (and reads nothing)
    idx.copy_(torch.tensor([len(store), -1], device=DEV))
    call()
    torch.cuda.synchronize()
    assert all(bool((o == 0).all()) for o in outs)


# ------------------------------------------------------------------ row edges
def test_length_zero_actions_row():
    """A sample whose actions / rewards are empty (general constructor): an all-pad row."""
    g = torch.Generator().manual_seed(7)
    lists = C.make_experience([torch.randint(0, 37, (n,), generator=g) for n in (5, 3, 4)], [0.5, -1.0, 2.0])
    lists["actions_ixs"][1] = lists["actions_ixs"][1][:0]
    lists["rewards"][1] = lists["rewards"][1][:0]
    store = store_of(lists)
    assert store[1].actions_ixs.numel() == 0 and store[1].rewards.numel() == 0
    for ix in ([0, 1, 2], [1, 0], [1], [1, 1]):  # [1]: a batch of width 0 in the A family
        assert_batch(collate(store, ix), C.collate(lists, ix))
    assert tuple(collate(store, [1]).rewards.shape) == (1, 0)


def test_last_sample_and_equal_entries(golden, stores):
    lists, store = fixture_lists(golden("ilql_store"), "a"), stores["a"]
    last = len(store) - 1
    for ix in ([last], [last, 5, last], [5] * 6, [last] * 4):
        assert_batch(collate(store, ix), C.collate(lists, ix))


# ------------------------------------------------------------------ loader
def test_loader_sequential(golden, stores):
    lists, store = fixture_lists(golden("ilql_store"), "a"), stores["a"]
    n = len(store)
    loader = store.create_loader(5, shuffle=False)
    assert len(loader) == 3 and len(store.create_loader(5, shuffle=False, drop_last=True)) == 2
    assert len(store.create_loader(4)) == 3 and len(store.create_loader(n)) == 1
    batches = list(loader)
    assert len(batches) == 3
    for k, b in enumerate(batches):
        assert_batch(b, C.collate(lists, list(range(5 * k, min(n, 5 * k + 5)))))
    dropped = list(store.create_loader(5, shuffle=False, drop_last=True))
    assert len(dropped) == 2 and all(b.input_ids.shape[0] == 5 for b in dropped)


def test_loader_shuffled(golden, stores):
    lists, store = fixture_lists(golden("ilql_store"), "a"), stores["a"]
    n = len(store)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(11)).tolist()
    assert sorted(perm) == list(range(n)) and perm != list(range(n))
    batches = list(store.create_loader(5, generator=torch.Generator().manual_seed(11)))  # shuffle is the default
    assert len(batches) == 3 and sum(b.input_ids.shape[0] for b in batches) == n
    for k, b in enumerate(batches):
        assert_batch(b, C.collate(lists, perm[5 * k:5 * k + 5]))
    dropped = list(store.create_loader(5, shuffle=True, generator=torch.Generator().manual_seed(11), drop_last=True))
    assert len(dropped) == 2
    for k, b in enumerate(dropped):
        assert_batch(b, C.collate(lists, perm[5 * k:5 * k + 5]))


# ------------------------------------------------------------------ errors
def test_errors(golden, stores):
    lists = fixture_lists(golden("ilql_store"), "b")
    for short, name in (("attention_mask", "attention_mask"), ("dones", "dones"), ("rewards", "rewards")):
        bad = {f: list(v) for f, v in lists.items()}
        bad[short][2] = bad[short][2][:-1]
        with pytest.raises(ValueError, match=f"sample 2.*{name}"):
            store_of(bad)
    with pytest.raises(ValueError, match="empty"):
        P.ILQLRolloutStorage([], [], [], [], [], [], device=DEV)
    ids = lists["input_ids"]
    raw = [0.0] * len(ids)
    for p in (int(ids[1].shape[0]), int(ids[1].shape[0]) + 3, 0):
        pl = [1] * len(ids)
        pl[1] = p
        with pytest.raises(ValueError, match="sample 1"):
            P.ILQLRolloutStorage.from_samples(ids, raw, pl, device=DEV)
    with pytest.raises(ValueError):
        P.ILQLRolloutStorage.from_samples(ids, raw[:-1], device=DEV)
    with pytest.raises(ValueError, match="ROCm"):
        P.ILQLRolloutStorage.from_samples(ids, raw, device="cpu")
    store = stores["b"]
    rows = np.array([0, 1], dtype=np.int64)
    with pytest.raises(ValueError, match="ROCm"):  # a CPU tensor given to the ABI wrapper
        store.collate(torch.from_numpy(rows), rows)
    for bad_rows in ([0, len(store)], [-1, 0]):
        r = np.array(bad_rows, dtype=np.int64)
        with pytest.raises(IndexError):
            store.collate(torch.from_numpy(r).to(DEV), r)


# ------------------------------------------------------------------ end to end
def test_store_batch_through_heads_and_loss():
    """H 16, V 37, B 4: a store batch through ILQLHeads.forward_for_loss and ILQLConfig.loss gives
    the loss and stats, bit for bit, of the same batch built by the restatement on the host and
    moved to the device."""
    H, V, B = 16, 37, 4
    g = torch.Generator().manual_seed(21)
    ids = [torch.randint(0, V, (n,), generator=g) for n in (6, 9, 3, 7, 5, 2)]
    lists = C.make_experience(ids, (3 * torch.randn(len(ids), generator=g) + 1).tolist(), [2, 1, 1, 4, 2, 1])
    store = store_of(lists)
    ix = [3, 1, 5, 0]
    assert len(ix) == B
    dev_batch = collate(store, ix)
    host = C.collate(lists, ix)
    host_batch = P.ILQLBatch(*[host[f].to(DEV) for f in C.FIELDS])
    torch.manual_seed(22)
    heads = P.ILQLHeads(P.ILQLConfig(), H, V).to(DEV)
    L = host["input_ids"].shape[1]
    hs = torch.randn(B, L, H, generator=g).to(DEV)
    logits = torch.randn(B, L, V, generator=g).to(DEV)
    res = []
    for batch in (dev_batch, host_batch):
        out = heads.forward_for_loss(hs, batch.input_ids, batch.states_ixs, batch.actions_ixs)
        loss, stats = heads.config.loss((logits, out), batch)
        torch.cuda.synchronize()
        res.append((loss.detach().cpu(), {k: torch.as_tensor(v).detach().cpu() for k, v in stats.items()}))
    (l0, s0), (l1, s1) = res
    assert bool(torch.isfinite(l0)) and same(l0, l1)
    assert list(s0) == list(P.ILQL_LOSS_KEYS) == list(s1)
    for k in s0:
        assert same(s0[k].float(), s1[k].float()), k
