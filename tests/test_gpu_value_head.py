"""The fused bf16 value head on the GPU (csrc/value_head.hip k_vhead, trlx_value_head_fwd / _bwd,
value_head.value_head / ValueHead) against the two CPU restatements of tests/value_head_checks.py.

Tolerance (not fixed in advance): for every case e_ref = max|(a) − (b)|, torch's bf16 CPU module
against the fp64 oracle on the same inputs; the kernel must satisfy
    max|kernel − (b)| <= 2·e_ref + 1e-6·max|(b)|
for the values and for each of dh, dW1, db1, dw2, db2 (see value_head_checks).

Shapes, automatic split count (on a 256-CU part every one of them gives each workgroup ONE
32-column slice, so one chunk and one epilogue): H in {32, 64, 160, 768} (one K step, one MFMA
column group, a ragged column slice, the product size) with N in {1, 65}, and N in {1, 63, 64, 65,
130} (one token, a partial block, an exact block, one and two over) with H = 64.

Shapes, forced split count S in {1, 2, 3} (value_head_checks.multi_chunk_cases: the training
shapes' geometry, several 128-column chunks per workgroup, at small N; S = 3 and S = 2 are what
C2 and the C3 shard get).  With nk = H/32 K steps a chunk, the stage ring's phase at a chunk
boundary is (chunk·nk) mod 3 and the b1 / w2 vector slot is chunk mod 3:
    H   96  nk  3 (mod 3 = 0)   2 chunks at S = 1 (128 + a ragged 64): the smallest multi-chunk walk
    H  128  nk  4 (1)           2 chunks: a step right after an epilogue, ring phase 1
    H  256  nk  8 (2)           4 chunks: the first reuse of a vector slot; S 2, 3: 2 chunks, ragged at 3
    H  288  nk  9 (0)           5 chunks, the last a ragged 64 after a slot reuse; S 2: 3, S 3: 2 chunks
    H  320  nk 10 (1)           5 chunks; S 2: 3 (ragged 64), S 3: 2 (ragged 64 / 96)
    H  448  nk 14 (2)           7 chunks: the vector ring wraps twice; S 2: 4 (ragged), S 3: 3 (ragged)
    H  768  nk 24 (0)           12 chunks, the product's H; S 2: 6 chunks (C3 shard), S 3: 4 (C2)
(H 96 and 128 only at S = 1: their S = 2, 3 slices are single chunks.)  N = 65 (two token blocks,
the second with one token) at every H; at H 256 and 768 also N = 1, N = 33 (the second half block
holds one token) and N = 130 (three blocks, the last with an empty half block that has to write
zero column sums).  Beside the tolerance rule, checks no tolerance can hide: the raw backward's dz,
dw2, db1, db2 are bit-identical for S in {1, 2, 3, cap} (a column's z has one K order whatever
slice or chunk holds it, dz is element-wise, the column sums run over tokens); with a one-hot w2
and b2 = 0 the fp32 values are relu(bf16(z_j)) and bit-identical over S; fp32 gradients round to
the bf16 ones; a row-strided h gives the contiguous backward's bits; guard elements past values,
dz, dw2, db1 stay intact.  Every raw call here starts from a workspace of NaN bit patterns.

TRLX_VALUE_HEAD_PARITY_OUT=<file>: the measured figures of the parity cases are written there
(profiles/value_head_parity.json is such a run; "S" is the forced split count, 0 = automatic).
"""
import json
import os
import sys

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import value_head_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VH = sys.modules["trlx_t5_amd.value_head"]
KEYS = ("h", "w1", "b1", "w2", "b2")
SHAPES = [(1, 32), (65, 32), (1, 64), (63, 64), (64, 64), (65, 64), (130, 64), (1, 160), (65, 160), (1, 768),
          (65, 768)]
MULTI = C.multi_chunk_cases()
MULTI_NH = sorted({(N, H) for N, H, _ in MULTI}, key=lambda k: (k[1], k[0]))
_REFS = {}
_FIGURES = {}


def refs(N, H):
    """The case's operands and both restatements, computed once and shared (never modified)."""
    if (N, H) not in _REFS:
        c = C.make_case(N, H, C.case_seed(N, H))
        args = [c[k] for k in KEYS]
        _REFS[(N, H)] = (c, C.reference_bf16(*args, dv=c["dv"]), C.oracle_fp64(*args, dv=c["dv"]))
    return _REFS[(N, H)]


def dev_ops(c, grad=False):
    return [c[k].to(DEV).requires_grad_(grad) for k in KEYS]


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


@pytest.fixture(scope="module", autouse=True)
def parity_figures():
    yield
    path = os.environ.get("TRLX_VALUE_HEAD_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "max|kernel - fp64 oracle| <= 2 * e_ref + 1e-6 * max|oracle|, "
                               "e_ref = max|torch bf16 CPU - fp64 oracle|",
                       "cases": [_FIGURES[k] for k in sorted(_FIGURES)]}, f, indent=1)


def parity(N, H, S):
    """Values and the five gradients through autograd under the rule; S = 0: the automatic split count."""
    c, a, b = refs(N, H)
    ops = dev_ops(c, grad=True)
    with _lib.tuning(vhead_splits=S):
        splits = P.value_head_splits(N, H)
        v = P.value_head(*ops)
        assert v.dtype == torch.float32 and tuple(v.shape) == (N,)
        v.backward(c["dv"].float().to(DEV))
        torch.cuda.synchronize()
    got = dict(values=v, dh=ops[0].grad, dw1=ops[1].grad, db1=ops[2].grad, dw2=ops[3].grad, db2=ops[4].grad)
    fig = {"N": N, "H": H, "S": S, "splits": splits}
    failed = []
    for k in ("values",) + C.GRADS:
        assert got[k] is not None, k
        if k != "values":   # a gradient has its tensor's dtype and shape
            assert got[k].dtype == torch.bfloat16 and got[k].shape == ops[C.GRADS.index(k)].shape
        e_ref, e_k = C.max_err(a[k], b[k]), C.max_err(got[k], b[k])
        lim = C.bound(e_ref, b[k])
        fig[k] = {"e_ref": e_ref, "e_kernel": e_k, "bound": lim, "max_abs": float(b[k].abs().max())}
        print(f"N={N} H={H} S={S} {k}: e_ref={e_ref:.6g} e_kernel={e_k:.6g} bound={lim:.6g}")
        if not e_k <= lim:
            failed.append(k)
    _FIGURES[(H, N, S)] = fig
    assert not failed, f"over the bound: {failed}: {fig}"
    return splits


@pytest.mark.parametrize("N,H", SHAPES)
def test_parity_values_and_gradients(N, H):
    assert parity(N, H, 0) == P.value_head_splits(N, H)


@pytest.mark.parametrize("N,H,S", MULTI)
def test_multi_chunk_parity_values_and_gradients(N, H, S):
    """Forward and backward at a forced split count that gives a workgroup two to twelve chunks
    (the header's table), under the unchanged rule."""
    assert max(C.chunks(H, S)) >= 2
    assert parity(N, H, S) == S


@pytest.mark.parametrize("S", [1, 2, 3, 64])
def test_forced_splits_reproducible_and_stride_independent(S):
    N, H = 65, 160
    c, a, b = refs(N, H)
    ops = dev_ops(c)
    with _lib.tuning(vhead_splits=S):
        s_eff = P.value_head_splits(N, H)
        assert s_eff == (S if S < 64 else 2 * H // 32)   # the cap: one split per 32 columns
        v1 = P.value_head(*ops)
        v2 = P.value_head(*ops)
        # the same rows through a [B, T, H] tensor's last position and behind a one-row offset
        g = torch.Generator().manual_seed(5)
        h3 = torch.randn(N, 3, H, generator=g).to(torch.bfloat16).to(DEV)
        h3[:, -1, :] = ops[0]
        view3 = h3[:, -1, :]
        big = torch.randn(N + 1, H, generator=g).to(torch.bfloat16).to(DEV)
        big[1:] = ops[0]
        view1 = big[1:]
        for view in (view3, view1):   # read in place, not through a copy
            assert not view.is_contiguous() or view.data_ptr() != big.data_ptr()
            assert VH._rows(view, H).data_ptr() == view.data_ptr()
        v3 = P.value_head(view3, *ops[1:])
        v4 = P.value_head(view1, *ops[1:])
        vb = P.value_head(*ops, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert view3.stride(0) == 3 * H and view1.data_ptr() == big.data_ptr() + 2 * H
    for other in (v2, v3, v4):
        assert torch.equal(bits(v1), bits(other))
    assert torch.equal(bits(vb), bits(v1.to(torch.bfloat16)))   # the fp32 result rounded once
    e_ref, e_k = C.max_err(a["values"], b["values"]), C.max_err(v1, b["values"])
    print(f"S={s_eff}: e_ref={e_ref:.6g} e_kernel={e_k:.6g}")
    assert e_k <= C.bound(e_ref, b["values"])
    assert P.value_head_splits(N, H) >= 1   # the knob is restored


def test_splits_are_a_function_of_the_shape():
    ncu = torch.cuda.get_device_properties(DEV).multi_processor_count
    for N, H in [(1, 768), (128, 768), (256, 768), (6144, 768), (12288, 768), (6144, 1024), (65, 32)]:
        want = max(1, min(-(-ncu // -(-N // 64)), 2 * H // 32, 64))
        assert P.value_head_splits(N, H) == want, (N, H)
    assert P.value_head_splits(128, 768) > 1 and 1 <= P.value_head_splits(6144, 768) <= 3
    assert 1 <= P.value_head_splits(12288, 768) <= 3
    assert P.value_head_splits(4, 48) == 0 and P.value_head_splits(0, 64) == 0


@pytest.mark.parametrize("N,H", [(65, 64), (1, 768)])
def test_output_dtype_rounds_once(N, H):
    c, _, _ = refs(N, H)
    ops = dev_ops(c)
    v32 = P.value_head(*ops)
    v16 = P.value_head(*ops, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert v16.dtype == torch.bfloat16 and torch.equal(bits(v16), bits(v32.to(torch.bfloat16)))


def nan_workspace(nbytes):
    """A workspace whose every fp32 is a NaN bit pattern: what a launch does not write shows."""
    return torch.full((max(int(nbytes), 4),), 0xFF, dtype=torch.uint8, device=DEV)


def raw_forward(ops, extra=0, out_dtype=torch.float32):
    """trlx_value_head_fwd itself into a [N + extra] tensor preset to 7."""
    h, w1, b1, w2, b2 = ops
    N, H = h.shape
    out = torch.full((N + extra,), 7.0, dtype=out_dtype, device=DEV)
    ws = nan_workspace(_lib.query("trlx_value_head_workspace_bytes", N, H))
    _lib.call("trlx_value_head_fwd", h.data_ptr(), h.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
              b2.data_ptr(), N, H, out.data_ptr(), _lib.dtype_code(out), ws.data_ptr(), _lib.stream_of(h))
    return out


def raw_backward(ops, dv, dv_dtype=None, grad_dtype=torch.bfloat16, extra_rows=0, extra=0):
    """trlx_value_head_bwd itself: (dz, dw2, db1, db2), preset to 7, dz with extra_rows rows and
    dw2 / db1 / db2 with `extra` elements beyond what the entry owns."""
    h, w1, b1, w2 = ops[:4]
    N, H = h.shape
    dz = torch.full((N + extra_rows, 2 * H), 7.0, dtype=torch.bfloat16, device=DEV)
    dw2 = torch.full((2 * H + extra,), 7.0, dtype=grad_dtype, device=DEV)
    db1 = torch.full((2 * H + extra,), 7.0, dtype=grad_dtype, device=DEV)
    db2 = torch.full((1 + extra,), 7.0, dtype=grad_dtype, device=DEV)
    ws = nan_workspace(_lib.query("trlx_value_head_bwd_workspace_bytes", N, H))
    _lib.call("trlx_value_head_bwd", h.data_ptr(), h.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
              dv.data_ptr(), _lib.dtype_code(dv) if dv_dtype is None else dv_dtype, N, H, dz.data_ptr(),
              dw2.data_ptr(), db1.data_ptr(), db2.data_ptr(), _lib.dtype_code(dw2), ws.data_ptr(), _lib.stream_of(h))
    return dz, dw2, db1, db2


def split_counts(H):
    return sorted({1, 2, 3, C.split_cap(H)})


@pytest.mark.parametrize("N,H", MULTI_NH)
def test_backward_bits_do_not_depend_on_the_split_count(N, H):
    """dz, dw2, db1 and db2 of the raw entry at S in {1, 2, 3, cap}: a column's z is the same MFMA
    K order in whatever slice and chunk it sits, dz is element-wise and the column sums run over
    the tokens in half-block order, so nothing may differ.  The cap is the one-chunk path of the
    automatic cases: the multi-chunk walk (epilogue stores in the queue of the next steps' DMAs,
    a reused vector slot, a ragged last chunk) is tied to it bit for bit."""
    c, _, b = refs(N, H)
    ops, dv = dev_ops(c), c["dv"].to(DEV)
    got = {}
    for S in split_counts(H):
        with _lib.tuning(vhead_splits=S):
            assert P.value_head_splits(N, H) == S
            got[S] = [bits(t) for t in raw_backward(ops, dv)]
    torch.cuda.synchronize()
    for S in split_counts(H)[1:]:
        for name, x, y in zip(("dz", "dw2", "db1", "db2"), got[1], got[S]):
            assert torch.equal(x, y), f"{name} at S={S} differs from S=1 in {int((x != y).sum())} elements"
    assert float((got[1][0] != 0).double().mean()) > 0.2   # not a row of sentinels or zeros


@pytest.mark.parametrize("H", [256, 288, 768])
def test_one_hot_w2_returns_the_column_for_every_split_count(H):
    """w2 = e_j, b2 = 0: v_t = relu(bf16(z_tj)) exactly (every other term is fma(r, 0, acc)), so
    the fp32 values are bit-identical over S in {1, 2, 3, cap} and meet the rule against the
    oracle, for the first and last column of every chunk and the column-group edges inside one:
    a wrong column, vector slot or mask that a random w2 averages away shows at its column."""
    N = 65
    c = dict(refs(N, H)[0])
    h, w1, b1 = (c[k].to(DEV) for k in ("h", "w1", "b1"))
    b2 = torch.zeros(1, dtype=torch.bfloat16)
    w2d, b2d = torch.zeros(1, 2 * H, dtype=torch.bfloat16, device=DEV), b2.to(DEV)
    z64 = c["h"].double() @ c["w1"].double().t() + c["b1"].double()
    want = torch.relu(z64.float().to(torch.bfloat16).double())
    failed = []
    for j in C.one_hot_columns(H):
        w2 = torch.zeros(1, 2 * H, dtype=torch.bfloat16)
        w2[0, j] = 1.0
        w2d.zero_()
        w2d[0, j] = 1.0
        got = {}
        for S in split_counts(H):
            with _lib.tuning(vhead_splits=S):
                got[S] = P.value_head(h, w1, b1, w2d, b2d)
        torch.cuda.synchronize()
        for S in split_counts(H)[1:]:
            assert torch.equal(bits(got[1]), bits(got[S])), (j, S)
        a = C.reference_bf16(c["h"], c["w1"], c["b1"], w2, b2)
        oracle = C.oracle_fp64(c["h"], c["w1"], c["b1"], w2, b2)["values"]
        assert torch.equal(oracle, want[:, j])
        e_ref, e_k = C.max_err(a["values"], oracle), C.max_err(got[1], oracle)
        print(f"one-hot H={H} j={j}: e_ref={e_ref:.6g} e_kernel={e_k:.6g} max={float(oracle.max()):.6g}")
        assert float(oracle.max()) > 0   # the column is live for some token
        if not e_k <= C.bound(e_ref, oracle):
            failed.append((j, e_ref, e_k))
    assert not failed, failed


def test_backward_dtypes_round_once():
    """grad_dtype F32: the three fp32 outputs, rounded to bf16 by torch, are the bf16 outputs; dv
    as fp32 holding the same bf16 numbers gives the bits of dv as bf16."""
    N, H = 65, 256
    c, _, b = refs(N, H)
    ops, dv = dev_ops(c), c["dv"].to(DEV)
    with _lib.tuning(vhead_splits=1):
        assert P.value_head_splits(N, H) == 1
        base = raw_backward(ops, dv)
        wide = raw_backward(ops, dv, grad_dtype=torch.float32)
        dv32 = raw_backward(ops, dv.float())
        both = raw_backward(ops, dv.float(), grad_dtype=torch.float32)
    torch.cuda.synchronize()
    for res in (wide, both):
        assert torch.equal(bits(res[0]), bits(base[0]))
        for name, x, y in zip(("dw2", "db1", "db2"), res[1:], base[1:]):
            assert x.dtype == torch.float32 and y.dtype == torch.bfloat16
            assert torch.equal(bits(x.to(torch.bfloat16)), bits(y)), name
    assert bool((wide[1] != wide[1].to(torch.bfloat16).float()).any())   # fp32 sums, not widened bf16
    for name, x, y in zip(("dz", "dw2", "db1", "db2"), dv32, base):
        assert x.dtype == torch.bfloat16 and torch.equal(bits(x), bits(y)), name
    # and the fp32 sums are nearer the oracle than their bf16 roundings may be
    for k, x in (("dw2", wide[1]), ("db1", wide[2]), ("db2", wide[3])):
        assert C.max_err(x, b[k]) <= C.max_err(x.to(torch.bfloat16), b[k]) + 1e-6 * float(b[k].abs().max()), k


@pytest.mark.parametrize("N,H,S", [(65, 256, 1), (65, 768, 2)])
def test_backward_reads_row_strided_h_in_place(N, H, S):
    """Autograd through h3[:, -1, :] of a [N, 3, H] tensor and through a view behind a one-row
    offset: all five gradients carry the contiguous case's bits, dh has the view's shape and
    nothing else of the base receives a gradient."""
    c, _, _ = refs(N, H)
    dv = c["dv"].float().to(DEV)
    g = torch.Generator().manual_seed(5)
    with _lib.tuning(vhead_splits=S):
        assert P.value_head_splits(N, H) == S
        ops = dev_ops(c, grad=True)
        P.value_head(*ops).backward(dv)
        want = [bits(t.grad) for t in ops]
        h3 = torch.randn(N, 3, H, generator=g).to(torch.bfloat16).to(DEV)
        h3[:, -1, :] = ops[0].detach()
        big = torch.randn(N + 1, H, generator=g).to(torch.bfloat16).to(DEV)
        big[1:] = ops[0].detach()
        for base, pick in ((h3, lambda t: t[:, -1, :]), (big, lambda t: t[1:])):
            base.requires_grad_(True)
            view = pick(base)
            view.retain_grad()
            assert tuple(view.shape) == (N, H) and VH._rows(view.detach(), H).data_ptr() == view.data_ptr()
            assert not view.is_contiguous() or view.data_ptr() != base.data_ptr()
            rest = dev_ops(c, grad=True)[1:]
            v = P.value_head(view, *rest)
            v.backward(dv)
            torch.cuda.synchronize()
            assert tuple(view.grad.shape) == (N, H) and view.grad.dtype == torch.bfloat16
            for name, x, t in zip(C.GRADS, want, [view] + rest):
                assert torch.equal(x, bits(t.grad)), name
            assert base.grad.shape == base.shape and torch.equal(bits(pick(base.grad)), want[0])
            outside = base.grad.clone()
            pick(outside).zero_()
            assert float(outside.float().abs().max()) == 0
    assert h3.stride(0) == 3 * H


@pytest.mark.parametrize("N,H,S", [(65, 288, 1), (130, 256, 2)])
def test_raw_entries_leave_guard_elements_intact(N, H, S):
    """values with N + 8 elements, dz with N + 1 rows, dw2 / db1 / db2 with 8 elements more: the
    sentinels in the excess survive, and what the entries own is what the exact-size call writes
    (a ragged last chunk whose masked columns lie past 2H at (65, 288, 1); an empty half block
    and the combine at (130, 256, 2))."""
    c, _, _ = refs(N, H)
    ops, dv = dev_ops(c), c["dv"].to(DEV)
    with _lib.tuning(vhead_splits=S):
        assert P.value_head_splits(N, H) == S
        v, vg = raw_forward(ops), raw_forward(ops, extra=8)
        v16 = raw_forward(ops, extra=8, out_dtype=torch.bfloat16)
        exact = raw_backward(ops, dv)
        guard = raw_backward(ops, dv, extra_rows=1, extra=8)
        guard32 = raw_backward(ops, dv, grad_dtype=torch.float32, extra_rows=1, extra=8)
    torch.cuda.synchronize()
    assert bool((vg[N:] == 7.0).all()) and torch.equal(bits(vg[:N]), bits(v))
    assert bool((v16[N:] == 7.0).all()) and torch.equal(bits(v16[:N]), bits(v.to(torch.bfloat16)))
    for res in (guard, guard32):
        dz, dw2, db1, db2 = res
        assert bool((dz[N:] == 7.0).all()) and torch.equal(bits(dz[:N]), bits(exact[0]))
        for name, x, y, n in (("dw2", dw2, exact[1], 2 * H), ("db1", db1, exact[2], 2 * H), ("db2", db2, exact[3], 1)):
            assert bool((x[n:] == 7.0).all()), name
            assert torch.equal(bits(x[:n].to(torch.bfloat16)), bits(y)), name
    assert not bool((exact[0] == 7.0).all(1).any())   # every dz row was written


@pytest.mark.parametrize("N,H,S", [(65, 64, 0), (65, 160, 3)])
def test_relu_mask_columns_contribute_nothing(N, H, S):
    """Columns whose z is exactly 0 (zero W1 row, b1 = 0) or negative (b1 = -1): nothing forward,
    dz = 0, dw2 = 0, db1 = 0 (torch's relu gradient at 0 is 0)."""
    c = dict(refs(N, H)[0])
    zero_cols = torch.tensor([0, 15, 16, 63, 64, 2 * H - 1])
    neg_cols = torch.tensor([1, 31, 65, 2 * H - 2])
    dead = torch.cat([zero_cols, neg_cols])
    c["w1"] = c["w1"].clone()
    c["b1"] = c["b1"].clone()
    c["w1"][dead] = 0
    c["b1"][zero_cols] = 0
    c["b1"][neg_cols] = -1
    args = [c[k] for k in KEYS]
    a, b = C.reference_bf16(*args, dv=c["dv"]), C.oracle_fp64(*args, dv=c["dv"])
    assert float(b["db1"][dead].abs().max()) == 0 and float(a["dw2"][dead].float().abs().max()) == 0
    with _lib.tuning(vhead_splits=S):
        ops = dev_ops(c, grad=True)
        v = P.value_head(*ops)
        # the dead columns' w2 does not matter: the same bits with it zeroed
        w2z = c["w2"].clone()
        w2z[0, dead] = 0
        vz = P.value_head(ops[0].detach(), ops[1].detach(), ops[2].detach(), w2z.to(DEV), ops[4].detach())
        v.backward(c["dv"].float().to(DEV))
        dz, dw2, db1, db2 = raw_backward([t.detach() for t in ops], c["dv"].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(v), bits(vz))
    e_ref, e_k = C.max_err(a["values"], b["values"]), C.max_err(v, b["values"])
    print(f"mask N={N} H={H}: e_ref={e_ref:.6g} e_kernel={e_k:.6g}")
    assert e_k <= C.bound(e_ref, b["values"])
    dead = dead.to(DEV)
    assert float(dz[:, dead].float().abs().max()) == 0
    assert float(dw2[dead].float().abs().max()) == 0 and float(db1[dead].float().abs().max()) == 0
    assert float(ops[3].grad[0, dead].float().abs().max()) == 0 and float(ops[2].grad[dead].float().abs().max()) == 0
    assert float(ops[1].grad[dead].float().abs().max()) == 0
    # the raw entry and autograd agree, and the live columns are live
    assert torch.equal(bits(dw2), bits(ops[3].grad.reshape(-1))) and torch.equal(bits(db1), bits(ops[2].grad))
    assert torch.equal(bits(db2), bits(ops[4].grad.reshape(-1)))
    live = torch.ones(2 * H, dtype=torch.bool, device=DEV)
    live[dead] = False
    assert float(dz[:, live].float().abs().max()) > 0
    # dz itself: bf16(dv·w2) under the oracle's mask, wherever the oracle's z is not within a
    # rounding of 0 (there the fp32 sum's sign may differ)
    z64 = c["h"].double() @ c["w1"].double().t() + c["b1"].double()
    want = (c["dv"].float()[:, None] * c["w2"].float()).to(torch.bfloat16)
    want = torch.where(z64.float().to(torch.bfloat16) > 0, want, torch.zeros_like(want))
    clear = (z64.abs() > 1e-4) | (z64 == 0)
    assert torch.equal(bits(dz)[clear], bits(want)[clear]) and float(clear.double().mean()) > 0.99


def test_autograd_contract():
    N, H = 65, 64
    c, a, b = refs(N, H)
    ops = dev_ops(c, grad=True)
    dv = c["dv"].float().to(DEV)
    v = P.value_head(*ops)
    assert v.requires_grad and v.grad_fn is not None
    v.backward(dv)
    assert all(t.grad is not None for t in ops)
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        v.backward(dv)
    # an in-place edit of w1 between forward and backward: autograd's version check
    ops = dev_ops(c, grad=True)
    v = P.value_head(*ops)
    with torch.no_grad():
        ops[1].mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        v.backward(dv)
    # no_grad: the same bits, nothing kept
    ops = dev_ops(c, grad=True)
    v_grad = P.value_head(*ops)
    with torch.no_grad():
        v_ng = P.value_head(*ops)
    assert not v_ng.requires_grad and v_ng.grad_fn is None
    assert torch.equal(bits(v_grad), bits(v_ng))
    # bf16 values take a bf16 gradient; retain_graph allows the second backward, same bits
    ops = dev_ops(c, grad=True)
    vb = P.value_head(*ops, out_dtype=torch.bfloat16)
    vb.backward(c["dv"].to(DEV), retain_graph=True)
    g1 = [t.grad.clone() for t in ops]
    for t in ops:
        t.grad = None
    vb.backward(c["dv"].to(DEV))
    torch.cuda.synchronize()
    for x, t in zip(g1, ops):
        assert torch.equal(bits(x), bits(t.grad))
    # only the tensors that ask get a gradient
    ops = dev_ops(c)
    ops[0].requires_grad_(True)
    P.value_head(*ops).backward(dv)
    assert ops[0].grad is not None and all(t.grad is None for t in ops[1:])


def test_module_is_a_drop_in():
    H = 64
    c, a, b = refs(130, H)
    head = P.ValueHead(H).to(DEV)
    head.load_state_dict({"0.weight": c["w1"], "0.bias": c["b1"], "2.weight": c["w2"], "2.bias": c["b2"]}, strict=True)
    h = c["h"].to(DEV).reshape(2, 65, H)
    out = head(h)
    assert tuple(out.shape) == (2, 65, 1) and out.dtype == torch.bfloat16
    assert torch.equal(bits(out), bits(head.values(h, torch.bfloat16)[..., None]))
    assert tuple(head.values(h).shape) == (2, 65) and head.values(h).dtype == torch.float32
    assert out.squeeze(-1).shape == (2, 65)
    e_ref, e_k = C.max_err(a["values"], b["values"]), C.max_err(head.values(h), b["values"])
    assert e_k <= C.bound(e_ref, b["values"])
    # the module trains: every parameter and the input receive a gradient
    h.requires_grad_(True)
    head(h).sum().backward()
    assert h.grad is not None and all(p.grad is not None and p.grad.shape == p.shape for p in head.parameters())
    assert isinstance(P.make_value_head(H, 1), P.ValueHead)


def test_decode_loop_records_the_fused_values():
    """B 4, T 6, V 37, H 64: the decode loop's per-step values land in the recorder as
    v_head.values(h_all) computes them in one go (same inputs, same splits)."""
    B, T, V, H = 4, 6, 37, 64
    g = torch.Generator().manual_seed(11)
    head = P.ValueHead(H).to(DEV)
    h_all = torch.randn(B, T, H, generator=g).to(torch.bfloat16).to(DEV)
    logits = torch.randn(B, T, V, generator=g).to(DEV)
    ref_logits = torch.randn(B, T, V, generator=g).to(DEV)
    rec = P.PPORolloutRecorder(B, T, DEV, pad_token_id=0, eos_token_id=None)
    with _lib.tuning(vhead_splits=2), torch.no_grad():
        for t in range(T):
            values = head.values(h_all[:, t, :])   # a row-strided view, read in place
            P.ppo_sample_step(logits[:, t], ref_logits=ref_logits[:, t], recorder=rec, values=values,
                              u=torch.rand(B, generator=g).to(DEV), cur_len=t)
        want = head.values(h_all)
    torch.cuda.synchronize()
    assert rec.t == T and tuple(want.shape) == (B, T)
    for t in range(T):
        assert torch.equal(bits(rec.values[:, t]), bits(want[:, t])), t


def test_guards_leave_outputs_untouched():
    N, H = 65, 64
    c, _, _ = refs(N, H)
    h, w1, b1, w2, b2 = dev_ops(c)
    out = torch.full((N,), 7.0, device=DEV)
    ws = torch.empty(_lib.query("trlx_value_head_workspace_bytes", N, H), dtype=torch.uint8, device=DEV)
    st = _lib.stream_of(h)

    def fwd(hp=None, ld=H, n=N, hh=H, dt=_lib.F32, w1p=None, b1p=None, wsp=ws.data_ptr(), outp=None):
        _lib.call("trlx_value_head_fwd", h.data_ptr() if hp is None else hp, ld,
                  w1.data_ptr() if w1p is None else w1p, b1.data_ptr() if b1p is None else b1p, w2.data_ptr(),
                  b2.data_ptr(), n, hh, out.data_ptr() if outp is None else outp, dt, wsp, st)

    bad = [dict(hh=48), dict(hh=0), dict(hh=8224), dict(n=0), dict(ld=H - 8), dict(ld=H + 4),
           dict(hp=h.data_ptr() + 2), dict(w1p=w1.data_ptr() + 8), dict(b1p=b1.data_ptr() + 2), dict(dt=_lib.I64),
           dict(dt=7)]
    for kw in bad:
        with pytest.raises(ValueError):
            fwd(**kw)
    with pytest.raises(ValueError):   # NULL h
        _lib.call("trlx_value_head_fwd", None, H, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), N, H,
                  out.data_ptr(), _lib.F32, ws.data_ptr(), st)
    with _lib.tuning(vhead_splits=2):
        with pytest.raises(ValueError):   # splits need the workspace
            fwd(wsp=None)
    with pytest.raises(ValueError):
        _lib.set_tuning("vhead_splits", 65)
    with pytest.raises(ValueError):
        _lib.set_tuning("vhead_splits", -1)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the wrapper's own checks, with device tensors
    for args in ([h.float(), w1, b1, w2, b2], [h, w1[:-1], b1, w2, b2], [h[:, :48], w1, b1, w2, b2],
                 [h, w1, b1, w2, b2.cpu()]):
        with pytest.raises((ValueError, TypeError)):
            P.value_head(*args)
    # backward: sentinels survive a refused call
    dv = c["dv"].to(DEV)
    for kw in (dict(dv_dtype=_lib.I64),):
        with pytest.raises(ValueError):
            raw_backward([h, w1, b1, w2], dv, **kw)
    with pytest.raises(ValueError):
        raw_backward([h[:, :48].contiguous(), w1, b1, w2], dv)
    keep = {}

    def sentinel_backward():
        dz = torch.full((N, 2 * H), 7.0, dtype=torch.bfloat16, device=DEV)
        small = torch.full((2 * H,), 7.0, dtype=torch.bfloat16, device=DEV)
        keep["t"] = (dz, small)
        _lib.call("trlx_value_head_bwd", h.data_ptr(), H, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                  dv.data_ptr(), _lib.BF16, N, H, dz.data_ptr(), small.data_ptr(), small.data_ptr(),
                  small.data_ptr(), _lib.BF16, None, st)   # NULL workspace

    with pytest.raises(ValueError):
        sentinel_backward()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in keep["t"])
    # and the operands are intact: the good call still gives the oracle's values
    fwd()
    torch.cuda.synchronize()
    _, a, b = refs(N, H)
    assert C.max_err(out, b["values"]) <= C.bound(C.max_err(a["values"], b["values"]), b["values"])
