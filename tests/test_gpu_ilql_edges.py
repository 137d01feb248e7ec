"""Edge suite of the ILQL loss (csrc/ilql_rows.hip: k_ilql_prep, k_ilql_rows, k_ilql_finalize)
against oracle.ppo_oracle.ilql_loss run in fp64 with its autograd.

  1  every entry of the launch table at its smallest and largest V, the table's boundaries, the
     four split instantiations and the split_lds / ilql_split knobs (which instantiation a V runs
     is proved on the CPU by tests/test_ilql_loss_table.py); the first V past the table refused
  2  logits and Q rows as views at every line shift 0..15 and head length 0..EPV-1, the gaps
     between the gradient rows untouched; gradient rows of another 16-B phase refused
  3  the action token at every store site of its gradient; permuted / repeated actions_ixs;
     indices outside the row give NaN rows and nothing else
  4  the prep / finalize grids: A != L-1, several blocks, the 128-block caps, the masked fast
     path decided by one zero weight in the last element
  5  bf16 vs / rewards, tau 0 and 1, the expectile tie, gathered target values, a NaN target

Bar (tests/ilql_loss_checks.py check64): fp32 rows rtol 1e-5 / atol 1e-6; bf16 rows rtol 1e-2 /
atol 2e-6 on the row gradients only, against fp64 on the bf16-quantised inputs.  The CPU file
shows that the fp32 oracle itself is inside the fp32 bar on every input set used here."""
import functools

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib

import ilql_loss_checks as C
from ilql_loss_checks import BF16, DEV, F32, FILL

pytestmark = pytest.mark.gpu
NAN = float("nan")


def tid(x):
    return {F32: "f32", BF16: "bf16"}.get(x, str(x))


def all_fill(*ts):
    return all(bool(((t._base if t._base is not None else t) == FILL).all()) for t in ts)


def outputs_untouched(o):
    return all_fill(o.dlogits, *o.dq, o.dvs, o.losses)


def inputs_unchanged(views, case):
    """The placed input rows still hold the case's values and their slack still holds FILL."""
    for k, v in views.items():
        src = case.logits if k == "logits" else case.qs[int(k[1])]
        if not torch.equal(v.cpu(), src):
            return False
        if v._base is not None:
            base, m = C.covered(v)
            if not bool((base[~m] == FILL).all()):
                return False
    return True


# ------------------------------------------------------------------ 1. launch table
@functools.lru_cache(maxsize=None)
def table_want(dtype, V, prompt, nq):
    return C.table_case(dtype, V, prompt, nq).want()


@pytest.mark.parametrize("dtype,V,split_lds,ilql_split", C.table_cases(), ids=tid)
def test_launch_table(dtype, V, split_lds, ilql_split):
    """One V of the table at B 2, L 4 with prompt 1 and 2 (nq 2; nq 1 for a few, ilql_loss_checks.table_nq): loss, the
    five stats and every gradient against fp64.  The rows sit 20 below zero with one peak each
    (ilql_loss_checks.rows_case), so a lane that is wrongly in or out of range moves the result
    by orders of magnitude more than the bar."""
    assert C.select(dtype, V, split_lds, ilql_split) is not None
    nq = C.table_nq(V, split_lds, ilql_split)
    with _lib.tuning(split_lds=split_lds, ilql_split=ilql_split):
        for prompt in (1, 2):
            c = C.table_case(dtype, V, prompt, nq)
            o, _ = C.launch_case(c)
            assert o.rc == 0, o.msg
            C.check64(C.got_of(o), table_want(dtype, V, prompt, nq), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=tid)
@pytest.mark.parametrize("split_lds", [0, 1])
def test_first_v_past_the_table_is_refused(dtype, split_lds):
    """V_LAST + 1 needs 16385 vectors with the shift margin: TRLX_ERR_SHAPE, no output written."""
    c = C.rows_case(1, 3, C.V_LAST[dtype] + 1, 77, dtype=dtype, peaks=False)
    with _lib.tuning(split_lds=split_lds):
        o, _ = C.launch_case(c, fn="trlx_ilql_rows")
        assert o.rc == C.ERR_SHAPE and "too long" in o.msg
        assert outputs_untouched(o)
        o, _ = C.launch_case(c)  # the fused entry: prep runs, the rows are refused
        assert o.rc == C.ERR_SHAPE and outputs_untouched(o)


# ------------------------------------------------------------------ 2. row phase
@functools.lru_cache(maxsize=None)
def phase_want(dtype, V):
    return C.phase_case(dtype, V).want()


PHASE_CASES = [(dt, V, 0) for dt in (F32, BF16) for V in C.PHASE_V[dt]] + [(F32, 51139, k) for k in (1, 2, 3)]


@pytest.mark.parametrize("dtype,V,ilql_split", PHASE_CASES, ids=tid)
def test_rows_at_every_shift_and_head(dtype, V, ilql_split):
    """logits, q0 and q1 as views into wider buffers: the rows of one launch cover every line
    shift 0..15 and every head length 0..EPV-1 (asserted from data_ptr() and the strides; q1 sits
    at another 256-B phase than q0).  V = 51139 is the largest split-path V, whose 12784 vectors
    at shift 15 end in the last lanes of the last LDS step; 65475 / 130951 are the largest
    register-resident V.  Gradients come back in grad_buffer_like buffers: the values against
    fp64, and every element between the rows as it was."""
    B, L, p0, sbb, stb = C.PHASE_LAYOUT[dtype]
    es = C.esize(dtype)
    c = C.phase_case(dtype, V)
    at = {"logits": (p0, sbb, stb), "q0": (p0, sbb, stb), "q1": (16 * 9 + es, sbb, stb)}
    with _lib.tuning(ilql_split=ilql_split):
        o, views = C.launch_case(c, at=at)
    assert o.rc == 0, o.msg
    for k, v in views.items():
        shifts, heads = C.phase_cover(v, L - 1)
        assert shifts == set(range(16)) and heads == set(range(16 // es)), (k, shifts, heads)
    for g, x in zip([o.dlogits] + o.dq, views.values()):  # the gradient rows repeat the rows' phases
        assert g.stride() == x.stride() and g.data_ptr() % 256 == x.data_ptr() % 256
    C.check64(C.got_of(o), phase_want(dtype, V), dtype)
    assert C.gaps_untouched(o) and inputs_unchanged(views, c)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=tid)
def test_gradient_rows_of_another_phase_are_refused(dtype):
    """dq / dlogits whose base or strides differ from the input's in 16-B phase:
    TRLX_ERR_STRIDE from the rows launch, nothing written."""
    c = C.rows_case(2, 4, 1031, 78, dtype=dtype, peaks=False)
    lg, q0 = c.logits.to(DEV), c.qs[0].to(DEV)

    def shifted(x, off, st_extra=0):  # x's shape in a FILL buffer, one element (or row stride) off
        B, T, V = x.shape
        buf = torch.full((x.numel() + B * T * st_extra + 512,), FILL, dtype=x.dtype, device=DEV)
        o0 = ((x.data_ptr() - buf.data_ptr()) % 256) // x.element_size() + off
        return buf.as_strided(x.shape, (T * (V + st_extra), V + st_extra, 1), o0)

    for kw in (dict(dqs=[shifted(q0, 0), shifted(q0, 1)]), dict(dqs=[shifted(q0, 1), shifted(q0, 0)]),
               dict(dlg=shifted(lg, 3)), dict(dlg=shifted(lg, 0, st_extra=1)), dict(dqs=[shifted(q0, 0, 1)] * 2)):
        for fn in ("trlx_ilql_rows", "trlx_ilql_loss_fused"):
            o, _ = C.launch_case(c, fn=fn, **kw)
            assert o.rc == C.ERR_STRIDE and "16-B phase" in o.msg, (kw.keys(), o.rc, o.msg)
            assert outputs_untouched(o)
    o, _ = C.launch_case(c, dqs=[shifted(q0, 0), shifted(q0, 0)], dlg=shifted(lg, 0))  # the same phase: accepted
    assert o.rc == 0
    C.check64(C.got_of(o), c.want(), dtype)


# ------------------------------------------------------------------ 3. position of the action token
YPOS_CASES = [(dt, V, 0) for dt in (F32, BF16) for V in C.YPOS_V[dt]] + [(F32, C.YPOS_V[F32][1], k) for k in (1, 2, 3)]


@pytest.mark.parametrize("dtype,V,ilql_split", YPOS_CASES, ids=tid)
def test_action_token_at_every_store_site(dtype, V, ilql_split):
    """B = 1, every row at head EPV-1 / shift 6 with EPV-1 tail elements; logits row k and the Q rows
    of action k have their token at position k of ilql_loss_checks.y_positions: each head and tail
    element, first / last element of body vector 0, the last body vector, step 0, the last VGPR
    step, and for the split kernels the first and last LDS step.  The full gradient rows against
    fp64: a misplaced gy shows as two wrong elements."""
    c, pos = C.ypos_case(dtype, V, ilql_split)
    p0 = C.ypos_p0(dtype)
    at = {k: (p0, 0, 0) for k in ("logits", "q0", "q1")}
    with _lib.tuning(ilql_split=ilql_split):
        o, views = C.launch_case(c, at=at)
    assert o.rc == 0, o.msg
    sel = C.select(dtype, V, 0, ilql_split)
    for v in views.values():  # the token list holds for every row as placed
        for p in C.row_ptrs(v)[0]:
            assert p % 256 == p0 and C.y_positions(p, V, dtype, sel) == pos
    sites = {C.locate(views["q0"].data_ptr(), V, dtype, sel, j)[:2] for j in pos.values()}
    want_sites = {("vgpr", 0), ("vgpr", sel[1] - 1)} | ({("lds", sel[1]), ("lds", sel[1] + sel[2] - 1)} if sel[2] else set())
    assert sites >= want_sites, sites
    want = c.want()
    C.check64(C.got_of(o), want, dtype)
    for k, j in enumerate(pos.values()):  # the action element itself, by name
        for got, ref in zip([o.dlogits] + o.dq, [want[2]] + want[3]):
            torch.testing.assert_close(got[0, k, j].double().cpu(), ref[0, k, j], msg=list(pos)[k], **C.bar(dtype))
    assert C.gaps_untouched(o)


@pytest.mark.parametrize("kind", ["perm", "repeat", "same"])
def test_actions_ixs_permuted_and_repeated(kind):
    c = C.perm_case(kind)
    o, _ = C.launch_case(c)
    assert o.rc == 0, o.msg
    C.check64(C.got_of(o), c.want(), F32)


@pytest.mark.parametrize("what", ["aix_neg", "aix_L1", "id_neg", "id_V", "id_V_prompt"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=tid)
def test_index_outside_the_row_gives_nan_rows_only(dtype, what):
    """actions_ixs outside [0, L-1) or a token outside [0, V): nothing is gathered, and exactly the
    rows that need that token are NaN — their gradient rows, their dvs entry, the losses their
    records feed.  Every other gradient equals the fp64 oracle on the batch with the
    index repaired (no other row's gradient depends on it); nothing else is written."""
    B, L, V, prompt = 3, 8, 37, 3
    clean = C.rows_case(B, L, V, 4100, dtype=dtype, prompt=prompt, offset=0.0, peaks=False)
    bad = clean.clone()
    b = bad.batch
    if what == "aix_neg":
        b.actions_ixs[1, 2] = -1
    elif what == "aix_L1":
        b.actions_ixs[1, 2] = L - 1
    elif what == "id_neg":
        b.input_ids[1, 4] = -1      # the next token of logits row (1, 3) and the token of action 1 (ix 3)
    elif what == "id_V":
        b.input_ids[1, 4] = V
    else:
        b.input_ids[1, 1] = V       # a prompt token: logits row (1, 0) only
    bad_l = {"id_neg": [(1, 3)], "id_V": [(1, 3)], "id_V_prompt": [(1, 0)]}.get(what, [])
    bad_q = {"aix_neg": [(1, 2)], "aix_L1": [(1, 2)], "id_neg": [(1, 1)], "id_V": [(1, 1)]}.get(what, [])
    wl, ws, wdl, wdq, wdv = clean.want()
    for bb, t in bad_l:
        wdl[bb, t] = NAN
        ws["loss_awac"] = ws["loss"] = wl = torch.tensor(NAN, dtype=torch.float64)
    for bb, a in bad_q:
        for g in wdq:
            g[bb, a] = NAN
        wdv[bb, a] = NAN
        wl = torch.tensor(NAN, dtype=torch.float64)
        for k in ("loss", "loss_q", "loss_v", "loss_cql"):
            ws[k] = wl
    p0 = 16 * 3 + C.esize(dtype)
    o, views = C.launch_case(bad, at={"logits": (p0, 20, 36), "q0": (p0, 20, 36)})
    assert o.rc == 0, o.msg
    C.check64(C.got_of(o), (wl, ws, wdl, wdq, wdv), dtype, equal_nan=True)
    assert C.gaps_untouched(o) and inputs_unchanged(views, bad)


# ------------------------------------------------------------------ 4. reductions
def run_loss(c, poison=None):
    """ILQLConfig.loss with autograd on the case (poison: a copy whose rows go to the GPU instead)."""
    src = poison or c
    cfg = P.ILQLConfig(two_qs=c.nq == 2, **c.hp)
    return C.run_gpu(cfg, src.logits, src.qs, src.tqs, src.vs, src.batch)


@pytest.mark.parametrize("variant", ["ragged", "ones"])
@pytest.mark.parametrize("name", [n for n in C.RED_SHAPES if not n.startswith("hot")])
def test_reduction_grids(name, variant):
    """ILQLConfig.loss at V 3 / 5 with A != L-1 (prompt 3 and prompt L-2): 2 prep blocks, exactly
    128, the 128-block cap (chunks of 257 for 32800 elements) and the finalize cap (147150 rows),
    with ragged masks and with no zero weight at all (the rows' fast path: no mask loads)."""
    c = C.red_case(name, variant)
    B, L = c.batch.input_ids.shape
    A = c.batch.actions_ixs.shape[1]
    assert A != L - 1
    full = int(c.batch.dones[:, :-1].sum()) == B * A and int(c.batch.attention_mask[:, 1:].sum()) == B * (L - 1)
    assert full == (variant == "ones")
    C.check64(run_loss(c), c.want(), F32)


@pytest.mark.parametrize("variant", ["done_zero", "attn_zero"])
@pytest.mark.parametrize("name", ["prep_multi_p3", "prep_multi_pL2", "prep_32800", "prep_32800_pL2"])
def test_one_zero_weight_in_the_last_element(name, variant):
    """Every weight one but dones[B-1, A-1] (or attention_mask[B-1, L-1]): prep's sums fall short of
    the counts by that one element of its last chunk, so the rows must load their masks and skip
    that row — it holds NaN here.  Outputs equal the fp64 oracle on the clean rows and the row's
    gradient is exact zeros.  Multi-block prep with A != L-1: the two index spaces end in
    different blocks."""
    c = C.red_case(name, variant)
    B, L = c.batch.input_ids.shape
    A = c.batch.actions_ixs.shape[1]
    short = (B * A - int(c.batch.dones[:, :-1].sum()), B * (L - 1) - int(c.batch.attention_mask[:, 1:].sum()))
    assert short == ((1, 0) if variant == "done_zero" else (0, 1))
    p = c.clone()
    if variant == "done_zero":
        for q in p.qs:
            q[B - 1, A - 1] = NAN
    else:
        p.logits[B - 1, L - 2] = NAN
    got = run_loss(c, poison=p)
    C.check64(got, c.want(), F32)
    rows = [q[B - 1, A - 1] for q in got[3]] if variant == "done_zero" else [got[2][B - 1, L - 2]]
    assert all(bool((r == 0).all()) for r in rows)


def test_zero_weight_rows_from_the_first_token():
    """A sequence that is padding from token 1 on: its logits row 0 is skipped like every other
    zero-weight row (all of them hold NaN), gradients exact zeros, outputs as the clean oracle."""
    c = C.mask_first_case()
    b = c.batch
    p = c.clone()
    lmask = torch.cat([b.attention_mask[:, 1:] == 0, torch.ones(3, 1, dtype=torch.bool)], dim=1)
    qmask = b.dones[:, :-1] == 0
    assert bool(lmask[1, 0]) and bool(qmask[1].all()) and not bool(lmask[0, :-1].any())
    p.logits[lmask] = NAN
    for q in p.qs:
        q[qmask] = NAN
    o, _ = C.launch_case(p)
    assert o.rc == 0, o.msg
    C.check64(C.got_of(o), c.want(), F32)
    assert bool((o.dlogits.cpu()[lmask] == 0).all()) and all(bool((q.cpu()[qmask] == 0).all()) for q in o.dq)


@pytest.mark.parametrize("name", ["prep_multi_p3", "prep_32800"])
def test_no_nonterminal_action(name):
    """Every done 0: n = max(1, 0), every Q row is skipped (all of them hold NaN) and written as
    zeros; loss_q = loss_v = loss_cql = 0 and the AWAC term as the oracle's."""
    c = C.red_case(name, "no_dones")
    p = c.clone()
    for q in p.qs:
        q.fill_(NAN)
    got = run_loss(c, poison=p)
    want = c.want()
    assert float(want[1]["loss_q"]) == 0.0 and float(want[1]["loss_cql"]) == 0.0
    C.check64(got, want, F32)
    assert all(bool((q == 0).all()) for q in got[3]) and bool((got[4] == 0).all())


def test_hot_path_twice_at_the_capped_grids():
    """ILQLHotPath.step at B 450, L 111, V 3: 148950 rows (finalize cap) and 49500 prep elements
    (prep cap), ragged.  Two calls on one hot path: bitwise equal, both tickets re-armed; against
    fp64."""
    c = C.red_case("hot_148950", "ragged")
    B, L = c.batch.input_ids.shape
    hp = P.ILQLHotPath(P.ILQLConfig(), B, L, 3, F32, DEV)
    bd = P.ILQLBatch(*(getattr(c.batch, f).to(DEV) for f in C.FIELDS))
    args = (c.logits.to(DEV), [q.to(DEV) for q in c.qs], [q.to(DEV) for q in c.tqs], c.vs.to(DEV).reshape(B, L), bd)
    outs = []
    R = B * L + 2 * B * (L - 1)
    assert R > 131072 and B * (L - 1) > 32768
    for _ in range(2):
        losses, dl, dq, dvs = hp.step(*args)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (losses, dl, *dq, dvs)])
        tick = hp.workspace[(16 + 16 * R + 15) // 16 * 16:][:16].view(torch.int32)
        assert int(tick.abs().sum()) == 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    losses, dl, dq0, dq1, dvs = outs[1]
    C.check64((losses[0], losses, dl, [dq0, dq1], dvs), c.want(), F32)


# ------------------------------------------------------------------ 5. scalars
@pytest.mark.parametrize("vs_bf16,rewards_bf16", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=tid)
def test_vs_and_rewards_in_bf16(dtype, vs_bf16, rewards_bf16):
    """ld_any: vs / rewards read as bf16, against fp64 on the quantised values."""
    c = C.scalar_case("plain", dtype=dtype)
    q = c.clone()
    if vs_bf16:
        q.vs = c.vs.bfloat16().float()
    if rewards_bf16:
        q.batch.rewards = c.batch.rewards.bfloat16().float()
    o, _ = C.launch_case(c, vs_dtype=BF16 if vs_bf16 else None, rewards_dtype=BF16 if rewards_bf16 else None)
    assert o.rc == 0, o.msg
    C.check64(C.got_of(o), q.want(), dtype)


@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_tau_at_its_ends(tau):
    c = C.scalar_case("plain")
    c.hp = dict(tau=tau, gamma=0.9, cql_scale=0.3, awac_scale=0.5)
    o, _ = C.launch_case(c)
    C.check64(C.got_of(o), c.want(), F32)
    assert float(c.want()[1]["loss_v"]) > 0


@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("tau", [0.0, 0.7, 1.0])
def test_expectile_tie_takes_the_upper_branch(nq, tau):
    """vs[2, 2] exactly the minimum target Q at its action: tQ >= V holds, weight tau (the term and
    its gradient are zero on either branch; the element must not turn NaN or pick up 1 - tau + tau)."""
    c = C.scalar_case("tie", nq=nq)
    c.hp = dict(tau=tau)
    o, _ = C.launch_case(c)
    want = c.want()
    C.check64(C.got_of(o), want, F32)
    assert float(o.dvs[2, 2]) == 0.0 and float(want[4][2, 2]) == 0.0


@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=tid)
def test_gathered_target_values_equal_the_row_form_bitwise(dtype, nq):
    """tq_gathered = 1 with fp32 [B, A] values taken at the action tokens: every output bitwise
    equal to the [B, A, V] row form (which is checked against fp64 here, nq = 1 included)."""
    c = C.scalar_case("plain", nq=nq, dtype=dtype)
    b = c.batch
    act = b.input_ids[:, 1:].gather(1, b.actions_ixs)
    gathered = [t.gather(-1, act[..., None]).squeeze(-1).float() for t in c.tqs]
    o, _ = C.launch_case(c)
    C.check64(C.got_of(o), c.want(), dtype)
    g, _ = C.launch_case(c, gathered_tq=gathered)
    assert g.rc == 0, g.msg
    for x, y in zip([o.losses, o.dlogits, *o.dq, o.dvs], [g.losses, g.dlogits, *g.dq, g.dvs]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("head", [0, 1])
def test_nan_target_q_at_one_action(head):
    """One target head NaN at the action of (2, 2): torch.minimum propagates it — loss_v (and the
    loss) NaN, that dvs entry NaN and no other."""
    c = C.scalar_case("plain")
    y = int(c.batch.input_ids[2, 1 + int(c.batch.actions_ixs[2, 2])])
    c.tqs[head][2, 2, y] = NAN
    o, _ = C.launch_case(c)
    want = c.want()
    assert bool(torch.isnan(want[1]["loss_v"])) and int(torch.isnan(want[4]).sum()) == 1
    C.check64(C.got_of(o), want, F32, equal_nan=True)
    assert int(torch.isnan(o.dvs).sum()) == 1 and bool(torch.isnan(o.dvs[2, 2]))
    assert not any(bool(torch.isnan(g).any()) for g in [o.dlogits] + o.dq)
