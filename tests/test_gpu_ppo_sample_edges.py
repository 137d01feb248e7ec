"""PPO rollout sampling step (csrc/ppo_sample.hip): every launch-table entry, search path and row
edge, against the fp64 oracle of tests/ppo_sample_checks.py or an expectation that is exact by
construction (the determinism case alone compares launches with each other).

  1  the launch table: live and shadowed entries, smallest / largest / first refused V
  2  sentinel rows: n logits tied at 0.0 over a background <= -40, top_k = n (or top_p = 0.5):
     u = (i + 0.5) / n returns the i-th sentinel exactly — head, every kind of body slot, tail
  3  EOS suppression with eos in the head, in vector step 0, a middle and the last step, the tail
  4  paths: ladder rows (a few logit levels with known multiplicities) whose kept set is exact;
     which search decides is predicted by ppo_sample_checks.list_path and asserted
  5  values: -inf entries, all-negative rows, +0.0 / -0.0 at the threshold, bf16 ties, temperature
  6  the log-prob of a near-certain token (the fp64 denominator's claim)
  7  bookkeeping and layout: finished rows of NaN, pad / eos = None, rows without a finite logit,
     B = 4096, B = 1, guard bands, rotating phases, determinism

Which path a case takes is known by reading the kernel only (nothing reports it at run time):
list_path restates the decision, the docstrings name the line of ppo_sample.hip that takes it.
Placed rows lie in poisoned buffers (+1e30 around every row); all outputs lie between guards."""
import math

import numpy as np
import pytest
import torch

from ppo_sample_checks import (BF16, DEV, F32, GUARD, LOGIT_POISON, NEG, OUT_DTYPES, TABLE, _lib,
                               check_draw_and_logprob, esize, line_ld, list_path, need, oracle_keep, place,
                               row_split, run_abi, select, suppress, thread_of)

pytestmark = pytest.mark.gpu
U_TOP = 1.0 - 2.0 ** -24   # the largest float32 below 1: torch.rand can return it


def dname(dtype):
    return "f32" if dtype == F32 else "bf16"


# ------------------------------------------------------------------ 1. the launch table
# (dtype, (vectors per thread, threads), smallest V, largest V): the live entries
LIVE = [(F32, (1, 1024), 1, 4035), (F32, (4, 1024), 4036, 16323), (F32, (8, 1024), 16324, 32707),
        (F32, (26, 512), 32708, 53187),
        (BF16, (1, 1024), 1, 8071), (BF16, (4, 1024), 8072, 32647), (BF16, (13, 512), 32648, 53127)]
FIRST_REFUSED = {F32: 53188, BF16: 53128}
SHAPES = [(d, e, v) for d, e, lo, hi in LIVE for v in (lo, hi)]


def shape_id(p):
    return f"{dname(p[0])}-N{p[1][0]}x{p[1][1]}-V{p[2]}"


def test_launch_table_live_entries_bounds_and_shadowed_entries():
    """LIVE and FIRST_REFUSED follow from the restated need(): every V up to the first refused one
    is walked.  F32T,16,512 and BF16T,8,512 are never selected: the 1024-thread entry walked
    before each accepts exactly the same V / EPV."""
    for dtype in (F32, BF16):
        spans, V = {}, 1
        while select(V, dtype) is not None:
            lo, hi = spans.get(select(V, dtype), (V, V))
            spans[select(V, dtype)] = (lo, V)
            assert hi in (V, V - 1), "an entry's V are not one interval"
            V += 1
        assert V == FIRST_REFUSED[dtype]
        assert [(dtype, e) + spans[e] for e in TABLE[dtype] if e in spans] == [r for r in LIVE if r[0] == dtype]
        assert all(select(v, dtype) is None for v in (V + 1, 2 * V, 10 * V))
    for dtype, dead, before in ((F32, (16, 512), (8, 1024)), (BF16, (8, 512), (4, 1024))):
        epv = 16 // esize(dtype)
        assert TABLE[dtype].index(before) < TABLE[dtype].index(dead)
        cap = [max(q for q in range(40000) if need(q * epv, epv, nt) <= n) for n, nt in (dead, before)]
        assert cap[0] == cap[1]
        live = {e for d, e, _, _ in LIVE if d == dtype}
        assert dead not in live and len(live) == len(TABLE[dtype]) - 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_first_refused_and_last_accepted_vocab(dtype):
    """The first refused V raises and writes nothing; one less launches (a sentinel at V - 1)."""
    V = FIRST_REFUSED[dtype]
    lg = torch.full((1, V), -40.0, dtype=dtype, device=DEV)
    u = torch.tensor([0.5], device=DEV)
    out = [torch.full((1,), GUARD, dtype=d, device=DEV) for d in OUT_DTYPES]
    with pytest.raises(ValueError):
        _lib.call("trlx_ppo_sample", lg.data_ptr(), V, _lib.dtype_code(lg), 1, V, 1.0, 1, 1.0, 1, 0, 0, -1, -1,
                  u.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None,
                  _lib.stream_of(lg))
    torch.cuda.synchronize()
    assert all(bool((o == GUARD).all()) for o in out)
    ok = lg[:, :V - 1]
    ok[0, V - 2] = 0.0
    ids, lp, mn, cnt = run_abi(ok, u, top_k=1)
    assert int(ids[0]) == V - 2 and int(cnt[0]) == 1 and float(mn[0]) == 0.0
    want = torch.log_softmax(ok.cpu().double(), -1)[0, V - 2]
    torch.testing.assert_close(lp.double()[0], want, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ 2. sentinel rows
def phases_for(dtype):
    """(head 0, shift 0), (head 0, shift 15), (head 1, shift 0), (head EPV - 1, shift 15)."""
    es = esize(dtype)
    return [0, 240, 240 + 16 - es, 224 + es]


def sentinel_positions(ph, V, dtype, entry):
    """Indices (ascending) that pin every kind of slot of a row at 256-B phase ph, and the set of
    vector steps they touch."""
    es, epv = esize(dtype), 16 // esize(dtype)
    n, nt = entry
    head, nvec, tail0, tail, shift = row_split(ph, V, es)
    js, steps = {0, V - 1}, set()
    if head:
        js.add(head - 1)
    if tail:
        js.add(tail0)
    if nvec:
        js |= {head, head + epv - 1, tail0 - 1}
        last = (nvec - 1 + shift) // nt
        for k in sorted({0, last // 2, last}):
            lo, hi = max(k * nt - shift, 0), min((k + 1) * nt - shift, nvec) - 1  # the step's vectors
            mid = min(lo + 3 * 64 + 5, hi)
            for i in ((lo, mid, hi) if last == 0 else (lo, hi) if k == last else (lo, mid)):  # different waves
                js.add(head + i * epv + i % epv)
                steps.add((i + shift) // nt)
        assert steps == {0, last // 2, last}
    assert len(js) <= 14
    return sorted(js), (head, nvec, tail0, tail, shift), steps


def check_exact(lg, rows, u, want, n, **kw):
    ids, lp, mn, cnt = run_abi(lg, u.to(DEV), **kw)
    assert ids.tolist() == want, (kw, [(w, g) for w, g in zip(want, ids.tolist()) if w != g])
    assert bool((cnt == n).all()) and bool((mn == 0.0).all()), (kw, cnt.tolist(), mn.tolist())
    ref = torch.log_softmax(rows.double(), -1)[torch.arange(len(want)), torch.tensor(want)]
    torch.testing.assert_close(lp.double(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype,entry,V", SHAPES, ids=[shape_id(p) for p in SHAPES])
def test_sentinel_rows_pin_exact_indices(dtype, entry, V):
    """Sentinels tied at 0.0, everything else in [-50, -40]: with top_k = n, or top_p = 0.5 alone
    (the ties at the nucleus boundary are all kept), the kept set is the n sentinels of weight
    exactly 1.0, so u = (i + 0.5) / n must return the i-th in index order, u = 0 the first and
    u = 1 - 2^-24 the last.  One-sentinel rows (n = 1, any u) pin index_of and the edge elements;
    the many-sentinel rows pin seg_pre, woff, the __shfl_up prefix and the in-thread pick.  At the
    largest V with shift 15 the last vector sits in the entry's last (thread, step) slot but 15."""
    assert select(V, dtype) == entry
    es, epv = esize(dtype), 16 // esize(dtype)
    ld = line_ld(V, dtype)
    g = torch.Generator().manual_seed(V)
    seen_shift, seen_head = set(), set()
    for ph in phases_for(dtype):
        js, geo, steps = sentinel_positions(ph, V, dtype, entry)
        head, nvec, tail0, tail, shift = geo
        n = len(js)
        assert shift + nvec <= entry[0] * entry[1]
        back = (-40.0 - 10.0 * torch.rand(n + 2, V, generator=g)).to(dtype)
        assert float(back.max()) <= -40.0
        one = back[:n].clone()
        one[torch.arange(n), torch.tensor(js)] = 0.0
        many = back.clone()
        many[:, js] = 0.0
        u_one = torch.rand(n, generator=g)
        u_many = torch.tensor([(i + 0.5) / n for i in range(n)] + [0.0, U_TOP], dtype=torch.float32)
        assert float(u_many[-1]) < 1.0
        for rows, u, want, k in ((one, u_one, js, 1), (many, u_many, js + [js[0], js[-1]], n)):
            lg = place(rows, ph, ld, LOGIT_POISON)
            B = rows.shape[0]
            assert row_split(lg.data_ptr(), V, es) == geo and row_split(lg[B - 1].data_ptr(), V, es) == geo
            check_exact(lg, rows, u, want, k, top_k=k)
            check_exact(lg, rows, u, want, k, top_k=0, top_p=0.5)
        seen_shift.add(shift)
        seen_head.add(head)
        if V >= 4096:  # threads of one step in different waves, and more than one element of a vector
            thr, step = thread_of(ph, V, dtype, entry[1])
            body = [j for j in js if head <= j < tail0]
            assert len({(int(step[j]), int(thr[j]) // 64) for j in body}) >= 3
            assert len({(j - head) % epv for j in body}) >= 3
    assert seen_shift == {0, 15} and seen_head == {0, 1, epv - 1} or V < epv


# ------------------------------------------------------------------ 3. EOS suppression
EOS_SHAPES = [p for p in SHAPES if p[2] > 1]


@pytest.mark.parametrize("dtype,entry,V", EOS_SHAPES, ids=[shape_id(p) for p in EOS_SHAPES])
def test_eos_suppressed_in_every_region(dtype, entry, V):
    """eos = +30 is every row's strict argmax, a runner-up of +20 sits elsewhere, top_k = 1.  While
    cur_len < min_length the token is the runner-up, with the log-prob of the unmodified row; at
    cur_len == min_length it is eos and `unfinished` clears.  eos lies in the head, in vector step
    0, a middle step, the last step (slot = q / EPV + shift, ks = slot / NT), the tail, at V - 1."""
    es, epv = esize(dtype), 16 // esize(dtype)
    n, nt = entry
    ld, B = line_ld(V, dtype), 4
    g = torch.Generator().manual_seed(V + 3)
    rows = torch.randn(B, V, generator=g).to(dtype)
    u = torch.rand(B, generator=g).to(DEV)
    hot, warm = torch.tensor(30.0, dtype=dtype), torch.tensor(20.0, dtype=dtype)
    regions = set()
    assert need(V, epv, nt) <= n
    for ph in phases_for(dtype):
        head, nvec, tail0, tail, shift = row_split(ph, V, es)
        last = (nvec - 1 + shift) // nt
        eoss = {V - 1: "end"}
        if head:
            eoss[head - 1] = "head"
        if tail:
            eoss[tail0] = "tail"
        for k in sorted({0, last // 2, last}):
            i = min(max(k * nt - shift, 0) + 70, min((k + 1) * nt - shift, nvec) - 1)
            eoss[head + i * epv + 1] = f"step{k}"
            assert (i + shift) // nt == k
        lg = place(rows, ph, ld, LOGIT_POISON)
        for eos, region in sorted(eoss.items()):
            regions.add(region)
            second = [r if r != eos else (r + 1) % V for r in (0, V - 1, V // 3, (eos + nt * epv) % V)]
            cpu = rows.clone()
            cpu[:, eos] = hot
            cpu[torch.arange(B), torch.tensor(second)] = warm
            keep_cols = lg[:, [eos] + second].clone()
            lg[:, eos] = hot.to(DEV)
            lg[torch.arange(B), torch.tensor(second)] = warm.to(DEV)
            ref = torch.log_softmax(cpu.double(), -1)
            unf = torch.ones(B, dtype=torch.int64, device=DEV)
            ids, lp, mn, cnt = run_abi(lg, u, top_k=1, cur_len=0, min_length=1, eos=eos, unfinished=unf)
            assert ids.tolist() == second, (ph, region, eos, ids.tolist(), second)
            assert bool((cnt == 1).all()) and bool((mn == 20.0).all()) and unf.tolist() == [1] * B
            torch.testing.assert_close(lp.double(), ref[torch.arange(B), torch.tensor(second)], rtol=1e-5, atol=1e-6)
            ids, lp, mn, cnt = run_abi(lg, u, top_k=1, cur_len=1, min_length=1, eos=eos, unfinished=unf)
            assert ids.tolist() == [eos] * B and unf.tolist() == [0] * B and bool((mn == 30.0).all())
            torch.testing.assert_close(lp.double(), ref[:, eos], rtol=1e-5, atol=1e-6)
            lg[:, [eos] + second] = keep_cols
    top = max((g[1] - 1 + g[4]) // nt for g in (row_split(ph, V, es) for ph in phases_for(dtype)))  # the last step
    assert regions >= {"end", "head", "tail"} | {f"step{k}" for k in (0, top // 2, top)}, regions


# ------------------------------------------------------------------ 4. ladder rows
LADDER = [(10.0, 1), (9.0, 3), (8.0, 10), (7.0, 30), (6.0, 100), (5.0, 300), (4.0, 1000), (3.0, 3000)]
FILL = (2.0, 1.5, 1.0, 0.5)   # every value is exact in bf16; the fill carries about 40 % of the mass at T = 1
CASE_SHAPES = [(F32, 20011), (F32, 50257), (BF16, 20011), (BF16, 50257)]   # N8x1024, N26x512, N4x1024, N13x512
case_shapes = pytest.mark.parametrize("dtype,V", CASE_SHAPES, ids=[f"{dname(d)}-V{v}" for d, v in CASE_SHAPES])
_rows = {}


def ladder_row(V, seed=0, levels=LADDER, fill=FILL, offset=0.0, peak=None):
    """fp32 [V]: the levels' values with their multiplicities, `fill` values elsewhere, scattered
    by a seeded permutation that puts the 2nd and 3rd largest entries at index 0 and V - 1."""
    key = (V, seed, tuple(levels), fill, offset, peak)
    if key not in _rows:
        g = torch.Generator().manual_seed(1000 + seed)
        vals = ([peak] if peak is not None else []) + [v for v, c in levels for _ in range(c)]
        vals = vals[:V]
        rest = torch.tensor(fill)[torch.randint(0, len(fill), (V - len(vals),), generator=g)]
        ordered = torch.cat([torch.tensor(vals), rest]) + offset
        perm = torch.randperm(V, generator=g)
        for rank, idx in ((1, 0), (2, V - 1)):
            if V > 2:
                pos = int((perm == idx).nonzero())
                perm[rank], perm[pos] = int(perm[pos]), int(perm[rank])
        x = torch.empty(V)
        x[perm] = ordered
        _rows[key] = x
    return _rows[key].clone()


def pick_p(x, T, top_k=0, min_keep=1, levels=None, target=None):
    """top_p (a float32 value) midway between the cumulative masses of two neighbouring levels of
    the top-k survivors of x (fp64 [V]): the nucleus is the `levels` highest levels (or the cut
    nearest to `target`).  Asserts the margin min |above - top_p * W| / W >= 1e-3 over every
    entry: no rounding of the kernel's fp32 masses (relative error about 1e-6) decides the set."""
    keep, _ = oracle_keep(x[None], T, top_k, 1.0, min_keep)
    vals, counts = torch.unique(x[keep[0]], return_counts=True)
    vals, counts = vals.flip(0), counts.flip(0)
    w = counts.double() * torch.exp((vals - vals[0]) / T)
    C = torch.cumsum(w, 0) / w.sum()
    above = torch.cat([torch.zeros(1, dtype=torch.float64), C[:-1]])
    if levels is None:
        levels = 1 + int(((above[:-1] + above[1:]) / 2 - target).abs().argmin())
    p = float(np.float32((float(above[levels - 1]) + float(above[levels])) / 2))
    margin = float((above - p).abs().min())
    assert margin >= 1e-3, (p, margin)
    return p


def ladder_case(dtype, V, row, T=1.0, top_k=0, top_p=1.0, min_keep=1, eos=None, path=None, scattered=True, B=4):
    """B copies of one row at u = 0, 1 - 2^-24 and random u, placed with a head, a tail and line
    shift 15: the kernel's kept set {x >= out_min_kept} and its count equal the oracle's bit for
    bit; draws and log-probs by the interval check.  Returns the oracle's kept set [V]."""
    es, epv = esize(dtype), 16 // esize(dtype)
    entry = select(V, dtype)
    rows = row.to(dtype).reshape(1, V).repeat(B, 1)
    u = torch.rand(B, generator=torch.Generator().manual_seed(V))
    u[0] = 0.0
    if B > 1:
        u[1] = U_TOP
    if V >= 2 * epv:
        h = max((h for h in range(1, epv) if (V - h) % epv), key=lambda h: (min(h, 2) + min((V - h) % epv, 2), h))
    else:
        h = 1
    lg = place(rows, 240 - h * es, line_ld(V, dtype), LOGIT_POISON)
    x = suppress(rows, eos)
    keep, w = oracle_keep(x, T, top_k, top_p, min_keep)
    got = list_path(x[0].float(), keep[0], lg.data_ptr(), dtype, entry, top_k, top_p, min_keep)
    assert path is None or got == path, (got, path)
    if scattered:  # the ladder's levels reach the head, every vector step and the tail
        thr, step = thread_of(lg.data_ptr(), V, dtype, entry[1])
        lvl = x[0] > float(torch.unique(x[0])[:len(FILL)].max())
        assert set(step[lvl].tolist()) == set(step.tolist()) and bool(lvl[0]) and bool(lvl[V - 1])
        assert int(step[0]) == -1 and int(step[V - 1]) == -1
    ids, lp, mn, cnt = run_abi(lg, u.to(DEV), T=T, top_k=top_k, top_p=top_p, min_keep=min_keep, eos=eos,
                               cur_len=0, min_length=0 if eos is None else 1)
    kept = (x >= mn.double().reshape(-1, 1)) & torch.isfinite(x)
    assert torch.equal(kept, keep), (int(kept[0].sum()), int(keep[0].sum()), mn.tolist())
    assert torch.equal(cnt.long(), keep.sum(-1))
    check_draw_and_logprob(rows, x, kept, w, ids, lp, u)
    return keep[0]


def entry_threads(dtype, V):
    return select(V, dtype)[1]


@case_shapes
def test_path_a_top_k_alone_on_the_list(dtype, V):
    """(a) k = 50: n0 = k <= NT (ppo_sample.hip:272), the 144 values >= the 50th fit the list
    (`n <= kPsCandCap`, :325), thr_k is ranked at :343.  Read from the code only."""
    keep = ladder_case(dtype, V, ladder_row(V), T=0.7, top_k=50, path="list")
    assert int(keep.sum()) == 144


@case_shapes
def test_path_b_top_k_with_the_list_overflowing_on_ties(dtype, V):
    """(b) k = 500 <= NT with 1000 values tied at the k-th: the list is tried (:272) and overflows
    (:325 fails), so nth_largest's count bisection runs (:374).  Read from the code only."""
    keep = ladder_case(dtype, V, ladder_row(V), T=0.7, top_k=500, path="overflow")
    assert int(keep.sum()) == 1444


@case_shapes
def test_path_c_top_k_above_the_thread_count(dtype, V):
    """(c) k = NT + 1: n0 > NT skips the list (:272), the count bisection runs (:374).  Read from
    the code only."""
    keep = ladder_case(dtype, V, ladder_row(V), T=0.7, top_k=entry_threads(dtype, V) + 1, path="skipped")
    assert int(keep.sum()) == 1444


@case_shapes
def test_path_d_small_nucleus_on_the_list(dtype, V):
    """(d) top-p alone, a nucleus of 14 tokens: n0 = the seed of 128 (:271), the list's smallest
    value is not kept (:362 not taken), the list decides (:368).  Read from the code only."""
    x = ladder_row(V)
    p = pick_p(x.double(), 1.0, levels=3)
    keep = ladder_case(dtype, V, x, top_p=p, path="list")
    assert int(keep.sum()) == 14


@case_shapes
def test_path_e_wide_nucleus_by_mass_bisection(dtype, V):
    """(e) top-p alone, a nucleus of 4444 tokens: the list's smallest value is kept (s_bad, :362),
    so the mass bisection over the whole row runs (:387 with thr_k = -inf).  Read from the code
    only."""
    x = ladder_row(V)
    p = pick_p(x.double(), 1.0, levels=8)
    keep = ladder_case(dtype, V, x, top_p=p, path="smallest-kept")
    assert int(keep.sum()) == 4444


@case_shapes
def test_path_f_top_k_and_nucleus_on_the_list(dtype, V):
    """(f) k = 50 (144 survivors) and a nucleus of 14 tokens inside them, W over the survivors
    (`top_k > 0 ? tot : w_all`, :360).  Read from the code only."""
    x = ladder_row(V)
    p = pick_p(x.double(), 1.0, top_k=50, levels=3)
    keep = ladder_case(dtype, V, x, top_k=50, top_p=p, path="list")
    assert int(keep.sum()) == 14


def combined_differs(x, k, p, keep):
    """On the oracle: top-k + top-p differs from top-k alone and from top-p alone on this row."""
    only_k, _ = oracle_keep(x.double()[None], 1.0, k, 1.0)
    only_p, _ = oracle_keep(x.double()[None], 1.0, 0, p)
    assert not torch.equal(keep, only_k[0]) and not torch.equal(keep, only_p[0])
    assert 1 < int(keep.sum()) < int(only_k.sum())


@pytest.mark.parametrize("k", [600, 2000])
@case_shapes
def test_path_g_top_k_and_nucleus_block_wide(dtype, V, k):
    """(g) k = 600 / 2000 with the nucleus strictly inside the top-k set: on the 1024-thread
    entries k = 600 tries the list and overflows (:325), otherwise n0 > NT skips it (:272); then
    thr_k by count bisection (:374), W = mass_ge(thr_k) (:380) and the nucleus bisection on
    mass_ge(fmaxf(cf, thr_k)) (:387).  Read from the code only."""
    x = ladder_row(V)
    p = pick_p(x.double(), 1.0, top_k=k, levels=5 if k == 600 else 6)
    path = "overflow" if k <= entry_threads(dtype, V) else "skipped"
    keep = ladder_case(dtype, V, x, top_k=k, top_p=p, path=path)
    assert int(keep.sum()) == (144 if k == 600 else 444)
    combined_differs(x, k, p, keep)


PEAK = 30.0   # one token with all but e^-18 of the mass: the nucleus of top_p = 0.5 is the peak alone


@pytest.mark.parametrize("kw,count,paths", [
    (dict(min_keep=3), 5, ("list", "list")),                      # 30, 10 and the three 9s tied at rank 3
    (dict(min_keep=3, top_k=600), 5, ("overflow", "skipped")),
    (dict(min_keep=3, top_k=2000), 5, ("skipped", "skipped")),
    (dict(min_keep=200), 445, (None, None)),                      # n0 = min_keep above the seed
    (dict(min_keep=1025), 1445, ("skipped", "skipped")),          # n0 above the thread count
    (dict(min_keep=5, top_k=2), 5, ("list", "list")),             # k raised to min_keep
    (dict(min_keep=5, top_k=2, top_p=1.0), 5, ("list", "list")),
], ids=["3-list", "3-k600", "3-k2000", "200", "1025", "k2-min5", "k2-min5-p1"])
@case_shapes
def test_path_h_min_tokens_to_keep_decides(dtype, V, kw, count, paths):
    """(h) a peaked row, top_p = 0.5: the nucleus is the peak, min_tokens_to_keep decides — on the
    list by `gt < a.min_keep` (:361), block-wide by `nth_largest(a.min_keep)` (:390); min_keep =
    200 makes n0 = min_keep (:271) and ends on either path (both give the 445 largest: the
    200th value has 300 ties), 1025 exceeds every thread count (:272), top_k = 2 is raised to
    min_keep = 5 by the launcher.  Read from the code only."""
    kw = dict(dict(top_p=0.5), **kw)
    path = paths[0 if entry_threads(dtype, V) == 1024 else 1]
    keep = ladder_case(dtype, V, ladder_row(V, peak=PEAK), path=path, **kw)
    assert int(keep.sum()) == count


@pytest.mark.parametrize("extra", [0, 1])
@case_shapes
def test_path_h_min_tokens_to_keep_of_the_whole_row(dtype, V, extra):
    """(h) min_tokens_to_keep = V and V + 1 (clamped to V by the launcher) on a peaked row with 100
    -inf entries: n0 = V skips the list (:272), nth_largest(V) finds fewer than V finite values
    and returns -inf (:390): every finite entry is kept.  Read from the code only."""
    x = ladder_row(V, peak=PEAK)
    x[torch.randperm(V, generator=torch.Generator().manual_seed(4))[:100] + 0] = NEG
    x[0], x[V - 1] = 9.0, 9.0
    keep = ladder_case(dtype, V, x, top_p=0.5, min_keep=V + extra, path="skipped", scattered=False)
    assert int(keep.sum()) == int(torch.isfinite(x).sum()) >= V - 100


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_path_i_rows_no_longer_than_the_seed(dtype):
    """(i) V <= 128 with top-p: n0 = 128 >= V skips the list (`int64_t(n0) < V`, :272) and the mass
    bisection runs; V = 1 and V = 2; top_k = V with top-p (no top-k threshold: thr_k = -inf at
    :374, W = mass_ge(-inf) at :380).  Read from the code only."""
    small = [(8.0, 1), (7.0, 2), (6.0, 5), (5.0, 12), (4.0, 30)]
    for V in (100, 128):
        x = ladder_row(V, levels=small, fill=(3.0, 2.5))
        for top_k in (0, V):
            p = pick_p(x.double(), 1.0, levels=3)
            keep = ladder_case(dtype, V, x, top_k=top_k, top_p=p, path="skipped", scattered=False)
            assert int(keep.sum()) == 8
    one = torch.tensor([3.0])
    assert int(ladder_case(dtype, 1, one, top_p=0.5, path="skipped", scattered=False).sum()) == 1
    assert int(ladder_case(dtype, 1, one, top_k=1, top_p=0.5, path="skipped", scattered=False).sum()) == 1
    two = torch.tensor([0.0, 1.0])   # masses 0.27 / 0.73
    assert ladder_case(dtype, 2, two, top_p=0.5, path="skipped", scattered=False).tolist() == [False, True]
    assert ladder_case(dtype, 2, two, top_p=0.9, path="skipped", scattered=False).tolist() == [True, True]
    assert ladder_case(dtype, 2, two, top_k=2, top_p=0.5, path="skipped", scattered=False).tolist() == [False, True]


@case_shapes
def test_eos_given_with_top_p_alone(dtype, V):
    """eos is the ladder's top token and suppressed: the kept set and its count are the oracle's
    on the suppressed row (the nucleus then starts at the three 9s)."""
    x = ladder_row(V)
    eos = int(x.argmax())
    sup = x.double().clone()
    sup[eos] = NEG
    p = pick_p(sup, 1.0, levels=3)
    keep = ladder_case(dtype, V, x, top_p=p, eos=eos, path="list", scattered=False)
    assert int(keep.sum()) == 43 and not bool(keep[eos])


# ------------------------------------------------------------------ 5. values
@pytest.mark.parametrize("kw,count", [(dict(top_k=400), 444), (dict(top_k=1025), 444), (dict(top_k=5000), 444),
                                      (dict(top_p="p"), 44), (dict(top_k=400, top_p="p"), 44)],
                         ids=["k400", "k1025", "k5000", "p", "k400-p"])
@case_shapes
def test_neg_inf_entries_are_never_kept(dtype, V, kw, count):
    """Only the 444 entries of the ladder's six highest levels are finite: k above the finite count
    keeps all of them (nth_largest returns -inf, ppo_sample.hip:255), -inf is never kept,
    counted or drawn; top-p alone and with such a k cuts inside the finite entries."""
    x = ladder_row(V)
    x[x < 5.0] = NEG
    kw = dict(kw)
    if "top_p" in kw:
        kw["top_p"] = pick_p(x.double(), 1.0, top_k=kw.get("top_k", 0), levels=4)
    keep = ladder_case(dtype, V, x, scattered=False, **kw)
    assert int(keep.sum()) == count and bool(torch.isfinite(x[keep]).all())


@pytest.mark.parametrize("case", ["a", "c", "e"])
@case_shapes
def test_all_negative_rows(dtype, V, case):
    """The ladder shifted by -40 (log-probs as logits) through (a), (c) and (e): negative floats
    have inverted keys (fkey, :47), the searches must order them as floats."""
    x = ladder_row(V, offset=-40.0)
    assert float(x.max()) == -30.0
    if case == "a":
        keep = ladder_case(dtype, V, x, T=0.7, top_k=50, path="list")
        assert int(keep.sum()) == 144
    elif case == "c":
        keep = ladder_case(dtype, V, x, T=0.7, top_k=entry_threads(dtype, V) + 1, path="skipped")
        assert int(keep.sum()) == 1444
    else:
        keep = ladder_case(dtype, V, x, top_p=pick_p(x.double(), 1.0, levels=8), path="smallest-kept")
        assert int(keep.sum()) == 4444


@pytest.mark.parametrize("kw,count", [(dict(top_k=100), 344), (dict(top_k=1025), 1444), (dict(top_p="zero"), 344),
                                      (dict(top_k=1025, top_p="four"), 344)], ids=["k100", "k1025", "p", "k1025-p"])
@case_shapes
def test_both_zeros_at_the_threshold(dtype, V, kw, count):
    """Levels 3, 2, 1 (44 entries), then 300 zeros — every second one -0.0 — then -1 and below:
    with the threshold at 0.0 both zeros are kept (float >=, where fkey(-0.0) < fkey(+0.0))."""
    levels = [(3.0, 1), (2.0, 3), (1.0, 40), (0.0, 300), (-1.0, 1100), (-2.0, 3000)]
    x = ladder_row(V, levels=levels, fill=(-3.0, -3.5, -4.0, -4.5))
    zeros = (x == 0.0).nonzero().reshape(-1)
    x[zeros[::2]] = -0.0
    assert int(torch.signbit(x[zeros]).sum()) == 150
    kw = dict(kw)
    if "top_p" in kw:
        kw["top_p"] = pick_p(x.double(), 1.0, top_k=kw.get("top_k", 0), levels=4)
    keep = ladder_case(dtype, V, x, **kw)
    assert int(keep.sum()) == count and bool(keep[zeros].all())


@pytest.mark.parametrize("k", [500, 600, 2000])
def test_bf16_rows_with_natural_ties(k):
    """N(0, 3) rounded to bf16 at V = 50257 (about 2000 distinct values, long runs of ties):
    k = 500 on the list or its overflow, k = 600 / 2000 with top-p block-wide, as (b) and (g)."""
    V = 50257
    x = (torch.randn(V, generator=torch.Generator().manual_seed(77)) * 3).to(BF16).float()
    if k == 500:
        ladder_case(BF16, V, x, T=0.7, top_k=k, scattered=False)
    else:
        p = pick_p(x.double(), 1.0, top_k=k, target=0.6)
        keep = ladder_case(BF16, V, x, top_k=k, top_p=p, path="skipped", scattered=False)
        combined_differs(x, k, p, keep)


@pytest.mark.parametrize("T", [0.05, 50.0])
@case_shapes
def test_temperature_extremes(dtype, V, T):
    """T = 0.05: only the maximum's three ties carry mass (the next level holds e^-20 each);
    T = 50: near uniform, the nucleus of about half the mass cuts inside the fill levels.
    top_p from pick_p at that T, same margin."""
    levels = [(10.0, 3)] + LADDER[1:]
    x = ladder_row(V, levels=levels)
    if T < 1:
        keep = ladder_case(dtype, V, x, T=T, top_p=pick_p(x.double(), T, levels=1), path="list")
        assert int(keep.sum()) == 3
        keep = ladder_case(dtype, V, x, T=T, top_k=50, path="list")
        assert int(keep.sum()) == 146
    else:
        keep = ladder_case(dtype, V, x, T=T, top_p=pick_p(x.double(), T, target=0.5), path="smallest-kept")
        assert int(keep.sum()) > 4446
        keep = ladder_case(dtype, V, x, T=T, top_k=2000, top_p=pick_p(x.double(), T, top_k=2000, target=0.5))
        assert 146 < int(keep.sum()) < 4446


# ------------------------------------------------------------------ 6. a near-certain token
def near_certain_rows(dtype, V):
    """Rows with |x| <= 16 whose token j leads by 12 to 16: (leader value, the others' range)."""
    g = torch.Generator().manual_seed(V)
    spec = [(16.0, (-16.0, 0.0), 0), (14.0, (-16.0, 0.0), V // 2), (12.0, (-16.0, -2.0), V - 1),
            (16.0, (-16.0, -8.0), 0), (13.0, (-16.0, -4.0), 1), (11.0, (-16.0, -3.0), V - 2)]
    rows = torch.empty(len(spec), V)
    for r, (top, (lo, hi), j) in enumerate(spec):
        rows[r] = lo + (hi - lo) * torch.rand(V, generator=g)
        rows[r, (j + 7) % V] = hi      # the runner-up: a lead of top - hi in [12, 16] ... [24]
        rows[r, j] = top
    return rows.to(dtype), [s[2] for s in spec]


@pytest.mark.parametrize("dtype,V", [(F32, 4035), (F32, 53187), (BF16, 8071), (BF16, 53127)],
                         ids=["f32-V4035", "f32-V53187", "bf16-V8071", "bf16-V53127"])
def test_logprob_of_a_near_certain_token(dtype, V):
    """top_k = 1 draws the leader; its log-prob, between about -3e-3 and -2e-8, must match fp64
    log_softmax of the stored values to rtol = 1e-5 with atol = 0 (the project's fp32 tolerance;
    each term's exponent argument carries at most about 2^-19 absolute error at |x| <= 16, 2e-6
    relative on the rest that the log-prob consists of).  This holds only if the maximum's own
    term is exactly 1: the parent's exponentials all carried the rounding of m * log2e (up to
    7e-7 relative, absolute on the log-prob) unless m was a power of two — leaders of 11 to 14 are
    here for that.  On the CPU: an fp32 running sum of the same terms in index order misses the
    tolerance on at least one row, so the rows do separate an fp32 denominator from fp64."""
    rows, lead = near_certain_rows(dtype, V)
    B = rows.shape[0]
    x = rows.double()
    want = torch.log_softmax(x, -1)[torch.arange(B), torch.tensor(lead)]
    assert bool((want < -1e-8).all()) and bool((want > -5e-2).all()), want
    terms = torch.exp(x - x.max(-1, keepdim=True).values).float().numpy()
    missed = 0
    for r in range(B):
        acc = np.float32(0.0)
        for t in terms[r]:
            acc = np.float32(acc + t)
        missed += abs(-math.log(float(acc)) - float(want[r])) > 1e-5 * abs(float(want[r]))
    assert missed >= 1
    lg = place(rows, 240 - esize(dtype), line_ld(V, dtype), LOGIT_POISON)
    ids, lp, mn, cnt = run_abi(lg, torch.rand(B, generator=torch.Generator().manual_seed(1)).to(DEV), top_k=1)
    assert ids.tolist() == lead
    print("log-probs", lp.tolist(), "relative error", ((lp.double() - want) / want).abs().tolist())
    torch.testing.assert_close(lp.double(), want, rtol=1e-5, atol=0.0)


# ------------------------------------------------------------------ 7. bookkeeping and layout
def gauss(B, V, dtype, seed, sigma=3.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, V, generator=g) * sigma).to(dtype)
    u = torch.rand(B, generator=g)
    u[0] = 0.0
    if B > 1:
        u[1] = U_TOP
    return x, u


def check_rows(rows, u, ids, lp, mn, cnt, T, top_k, eos=None):
    """Top-k rows against the oracle: exact kept set, count, draw interval, log-prob."""
    x = suppress(rows, eos)
    keep, w = oracle_keep(x, T, top_k, 1.0)
    kept = (x >= mn.double().reshape(-1, 1)) & torch.isfinite(x)
    assert torch.equal(kept, keep) and torch.equal(cnt.long(), keep.sum(-1))
    check_draw_and_logprob(rows, x, kept, w, ids, lp, u)


def test_finished_rows_of_nan_are_not_read():
    """Finished rows hold NaN: they give pad / 0 / 0 / 0 and stay finished; the live rows are the
    oracle's (so no NaN reached them)."""
    B, V, eos, pad, k = 6, 1031, 7, 3, 20
    rows, u = gauss(B, V, F32, 70)
    start = torch.tensor([1, 0, 1, 1, 0, 1])
    live = start == 1
    rows[~live] = float("nan")
    unf = start.clone().to(DEV)
    ids, lp, mn, cnt = run_abi(place(rows, 12, V + 3, LOGIT_POISON), u.to(DEV), T=0.7, top_k=k, eos=eos, pad=pad,
                               cur_len=5, min_length=0, unfinished=unf)
    assert ids[~live].tolist() == [pad, pad] and lp[~live].tolist() == [0, 0] and mn[~live].tolist() == [0, 0]
    assert cnt[~live].tolist() == [0, 0]
    assert torch.equal(unf.cpu(), (live & (ids != eos)).long())
    check_rows(rows[live], u[live], ids[live], lp[live], mn[live], cnt[live], 0.7, k)


def test_pad_and_eos_of_none():
    """pad_token_id = None: a finished row gets token 0 (documented), with and without `unfinished`
    (without it every row is live).  eos_token_id = None with `unfinished`: left untouched, even
    where it holds values other than 0 / 1."""
    B, V, k = 4, 1031, 5
    rows, u = gauss(B, V, F32, 71)
    lg, ud = rows.to(DEV), u.to(DEV)
    unf = torch.tensor([1, 0, 1, 0], device=DEV)
    ids, lp, mn, cnt = run_abi(lg, ud, top_k=k, eos=9, pad=None, unfinished=unf)
    live = torch.tensor([True, False, True, False])
    assert ids[~live].tolist() == [0, 0] and cnt[~live].tolist() == [0, 0] and lp[~live].tolist() == [0, 0]
    assert torch.equal(unf.cpu(), (live & (ids != 9)).long())
    check_rows(rows[live], u[live], ids[live], lp[live], mn[live], cnt[live], 1.0, k)
    ids, lp, mn, cnt = run_abi(lg, ud, top_k=k, eos=9, pad=None)
    check_rows(rows, u, ids, lp, mn, cnt, 1.0, k)
    odd = torch.tensor([1, 0, 5, -2], device=DEV)   # 0 = finished, anything else = live
    ids, lp, mn, cnt = run_abi(lg, ud, top_k=k, eos=None, pad=2, unfinished=odd)
    assert odd.tolist() == [1, 0, 5, -2] and int(ids[1]) == 2 and int(cnt[1]) == 0
    keep3 = torch.tensor([True, False, True, True])
    check_rows(rows[keep3], u[keep3], ids[keep3], lp[keep3], mn[keep3], cnt[keep3], 1.0, k)


@pytest.mark.parametrize("pad,eos", [(4, 4), (4, 9), (None, 0), (None, 9)])
def test_row_without_a_finite_logit_and_unfinished(pad, eos):
    """Documented in include/trlx_t5_amd.h: such a row returns pad (token 0 without one), writes 0
    to the other outputs, and `unfinished &= token != eos` holds for it as for any row: a pad that
    equals eos finishes the row (HF: a sequence ends at eos), any other pad leaves it live."""
    B, V = 4, 700
    rows = torch.full((B, V), NEG)
    rows[1] = torch.randn(V, generator=torch.Generator().manual_seed(2))
    rows[3, eos] = 1.0   # only eos is finite, and it is suppressed
    unf = torch.ones(B, dtype=torch.int64, device=DEV)
    u = torch.full((B,), 0.3)
    ids, lp, mn, cnt = run_abi(rows.to(DEV), u.to(DEV), cur_len=0, min_length=2, eos=eos, pad=pad, unfinished=unf)
    tok = 0 if pad is None else pad
    empty = torch.tensor([True, False, True, True])
    assert ids[empty].tolist() == [tok] * 3 and cnt[empty].tolist() == [0] * 3
    assert lp[empty].tolist() == [0.0] * 3 and mn[empty].tolist() == [0.0] * 3
    assert unf.cpu()[empty].tolist() == [int(tok != eos)] * 3
    assert int(unf[1]) == 1 and int(ids[1]) != eos and int(cnt[1]) == V - 1
    x = suppress(rows[1:2], eos)
    check_draw_and_logprob(rows[1:2], x, torch.isfinite(x), oracle_keep(x, 1.0, 0, 1.0)[1], ids[1:2], lp[1:2], u[1:2])


def test_large_batch_every_row_checked():
    B, V, k = 4096, 23, 5
    rows, u = gauss(B, V, F32, 50)
    ids, lp, mn, cnt = run_abi(rows.to(DEV), u.to(DEV), T=0.7, top_k=k)
    check_rows(rows, u, ids, lp, mn, cnt, 0.7, k)


@pytest.mark.parametrize("dtype,V", [(F32, 1031), (BF16, 50257)], ids=["f32-V1031", "bf16-V50257"])
def test_single_row_batch(dtype, V):
    rows, u = gauss(1, V, dtype, 51)
    ids, lp, mn, cnt = run_abi(place(rows, 16 - esize(dtype), V, LOGIT_POISON), u.to(DEV), T=0.7, top_k=20)
    check_rows(rows, u, ids, lp, mn, cnt, 0.7, 20)


@pytest.mark.parametrize("dtype,V", [(F32, 1031), (F32, 4099), (BF16, 2053), (BF16, 32771)],
                         ids=["f32-V1031", "f32-V4099", "bf16-V2053", "bf16-V32771"])
def test_odd_row_stride_rotates_the_phase(dtype, V):
    """ld_logits = V with V odd: every row has another 16-B phase (head, tail and line shift
    change from row to row).  Top-k rows, exact kept sets."""
    B, es = 16, esize(dtype)
    rows, u = gauss(B, V, dtype, 52 + V)
    lg = place(rows, 0, V, LOGIT_POISON)
    heads = {row_split(lg[b].data_ptr(), V, es)[0] for b in range(B)}
    assert len(heads) == 16 // es
    ids, lp, mn, cnt = run_abi(lg, u.to(DEV), T=0.7, top_k=20)
    check_rows(rows, u, ids, lp, mn, cnt, 0.7, 20)


def test_repeated_launches_are_bit_equal():
    """The one case that compares the kernel with itself: (f)'s and (g)'s rows and a Gaussian
    top-k + top-p row at V = 50257 (the candidate list is filled in the order the waves arrive, its
    masses are summed in list order), 20 launches each: all four outputs bit-equal every time."""
    V = 50257
    x = ladder_row(V)
    cases = [(x, dict(top_k=50, top_p=pick_p(x.double(), 1.0, top_k=50, levels=3))),
             (x, dict(top_k=600, top_p=pick_p(x.double(), 1.0, top_k=600, levels=5))),
             (x, dict(top_k=2000, top_p=pick_p(x.double(), 1.0, top_k=2000, levels=6)))]
    for dtype in (F32, BF16):
        grow, u = gauss(8, V, dtype, 90)
        lg = grow.to(DEV)
        runs = [(lg, u.to(DEV), dict(T=0.9, top_k=50, top_p=0.9))]
        for row, kw in cases:
            runs.append((row.to(dtype).reshape(1, V).repeat(8, 1).to(DEV), u.to(DEV), kw))
        for lgd, ud, kw in runs:
            first = run_abi(lgd, ud, **kw)
            for _ in range(19):
                again = run_abi(lgd, ud, **kw)
                for a, b in zip(first, again):
                    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), kw
