"""Global-norm gradient clipping on the GPU (trlx_grad_norm, trlx_adamw_step_clipped,
clip_grad_norm_, FusedAdamW.step(max_grad_norm=), adamw_step(max_grad_norm=),
ILQLHeads.step_and_sync(max_grad_norm=)).

The norm is checked against float32(sqrt(Σ g.double()²)) taken on the CPU to one fp32 ulp: the
kernel accumulates in fp64, whose relative error after n additions (n·2^-53) is far below 2^-24,
so only the final rounding to fp32 (and, at a tie, its direction) remains.  The coefficient and
the scaled gradients are torch's own ops on the device, bit for bit; the folded step is the
two-call route, bit for bit; ten steps meet adamw_checks' rule against the fp64 oracle that
clips in fp64 (grad_clip_checks).  TRLX_GRAD_CLIP_PARITY_OUT=<file>: the measured errors are
appended there (profiles/grad_clip_parity.json is such a run).

Sizes: 1, 5, one below / at / above one workgroup's chunk, more than three chunks; a list one
longer than the table (two launches under one norm); a list that mixes fp32 and bf16 gradients
with a zero-length tensor and a parameter without gradient.
"""
import copy
import json
import math
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
from trlx_t5_amd import optim as O
import adamw_checks as C
import grad_clip_checks as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = _lib.ADAMW_CHUNK
SIZES = [1, 5, CHUNK - 1, CHUNK, CHUNK + 11, 3 * CHUNK + 7]
OFFSETS = (0, 1, 3, 5, 7)
SENTINEL = 12345.0
HYPER = dict(lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=1e-2)


def phased(t, offset, pad=24):
    """A copy of `t` as a view at element `offset` of a larger sentinel-filled buffer."""
    buf = torch.full((t.numel() + pad,), SENTINEL, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()]
    view.copy_(t)
    return buf, view


def take_record(grads, max_norm, scale=0):
    """trlx_grad_norm on `grads` into a fresh record (float32[8] on the device)."""
    rec = torch.zeros(O.RECORD_FLOATS, dtype=torch.float32, device=DEV)
    ws = torch.empty(O._workspace_bytes(grads) // 8, dtype=torch.float64, device=DEV)
    O._grad_norm(grads, float(max_norm), rec, ws, scale)
    return rec


def fields(rec):
    raw = rec.detach().cpu()
    return {"norm": float(raw[0]), "coef": float(raw[1]), "nonfinite": int(raw.view(torch.int32)[2]),
            "sumsq": float(raw.view(torch.float64)[2])}


def bits(t):
    """The tensor's bytes as integers: equality of these is bit equality, NaNs included."""
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def cpu_norm32(grads):
    """float32(sqrt(Σ g.double()²)) on the CPU, as a Python float."""
    return float(torch.tensor(G.norm64(grads), dtype=torch.float64).float())


def assert_within_one_ulp(got, want, what):
    print(what, "norm", got, "cpu", want, "distance in ulp", abs(got - want) / G.f32_ulp(want))
    assert math.isfinite(got) and abs(got - want) <= G.f32_ulp(want), (what, got, want)


def gradient(n, seed, dtype, magnitude=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * magnitude).to(dtype)


# ------------------------------------------------------------------ the norm
@pytest.mark.parametrize("magnitude", [1.0, 1e20])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
def test_norm_is_within_one_ulp_at_every_size_and_phase(n, dtype, magnitude):
    """Element offsets 0, 1, 3, 5, 7 (every head length of fp32, odd 2-B phases of bf16); at 1e20
    an fp32 square overflows while the norm is finite.  Two runs give the same record bytes, the
    guards around the gradient stay, the gradient is only read."""
    g0 = gradient(n, 40 + n % 7, dtype, magnitude)
    want = cpu_norm32([g0])
    assert math.isfinite(want)
    for off in OFFSETS:
        buf, g = phased(g0, off)
        rec = take_record([g], math.inf)
        again = take_record([g], math.inf)
        f = fields(rec)
        assert_within_one_ulp(f["norm"], want, f"n={n} {dtype} x{magnitude} offset {off}")
        assert f["nonfinite"] == 0 and f["coef"] == 1.0  # max_norm = inf: the norm only
        assert abs(f["sumsq"] - G.norm64([g0]) ** 2) <= 1e-12 * f["sumsq"]
        assert same_bits(rec, again)
        assert torch.equal(g.cpu(), g0)
        assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


def many_small(count, seed=50):
    return [gradient(5 + (i % 3), seed + i, torch.float32) for i in range(count)]


def mixed_list():
    """fp32 and bf16 gradients in one list, a zero-length one among them."""
    return [gradient(CHUNK + 11, 60, torch.float32), gradient(5, 61, torch.bfloat16),
            torch.zeros(0), gradient(2 * CHUNK + 3, 62, torch.bfloat16), gradient(7, 63, torch.float32)]


@pytest.mark.parametrize("case", ["33 tensors", "mixed dtypes", "every size"])
def test_norm_over_a_list(case):
    grads = {"33 tensors": many_small(_lib.ADAMW_MAX_TENSORS + 1), "mixed dtypes": mixed_list(),
             "every size": [gradient(n, 70 + i, torch.float32) for i, n in enumerate(SIZES)]}[case]
    dev = [g.to(DEV) for g in grads]
    rec, again = take_record(dev, math.inf), take_record(dev, math.inf)
    assert_within_one_ulp(fields(rec)["norm"], cpu_norm32(grads), case)
    assert same_bits(rec, again)
    # the same list through clip_grad_norm_ with a parameter that has no gradient
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in dev] + [torch.nn.Parameter(torch.zeros(3, device=DEV))]
    for p, g in zip(ps, dev):
        p.grad = g.clone()
    total = P.clip_grad_norm_(ps, math.inf)
    assert total.shape == () and total.dtype == torch.float32 and total.device == DEV
    assert same_bits(total, rec[0]) and ps[-1].grad is None
    for p, g in zip(ps, dev):
        assert same_bits(p.grad, g)  # coef 1: torch multiplies by 1, the bits stay


# ------------------------------------------------------------------ the coefficient
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_coefficient_is_torchs_expression_on_the_device(dtype):
    g = gradient(CHUNK + 11, 80, dtype).to(DEV)
    norm = cpu_norm32([g])
    for max_norm in (2.0 * norm, 1e6, 0.37 * norm, 1.0, 1e-3, 0.0):
        rec = take_record([g], max_norm)
        want = torch.clamp(max_norm / (rec[0] + 1e-6), max=1.0)
        print(dtype, "max_norm", max_norm, "coef", float(rec[1]), "torch", float(want))
        assert same_bits(rec[1], want), (max_norm, float(rec[1]), float(want))
        if max_norm > norm:
            assert float(rec[1]) == 1.0
        else:
            assert float(rec[1]) < 1.0
        assert fields(rec)["nonfinite"] == 0


# ------------------------------------------------------------------ the in-place clip
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [5, CHUNK + 11, 3 * CHUNK + 7])
def test_clip_grad_norm_scales_in_place_as_torch_mul(dtype, n):
    g0 = gradient(n, 90, dtype)
    other0 = gradient(CHUNK - 1, 91, torch.float32)  # a second tensor: the norm is the global one
    for off in OFFSETS:
        buf, g = phased(g0, off)
        obuf, other = phased(other0, (off + 2) % 8)
        ps = [torch.nn.Parameter(torch.zeros(n, dtype=dtype, device=DEV)),
              torch.nn.Parameter(torch.zeros(CHUNK - 1, device=DEV))]
        ps[0].grad, ps[1].grad = g, other
        want_g, want_o = g.clone(), other.clone()
        total = P.clip_grad_norm_(ps, 0.5)
        rec = total._base  # the returned norm is a view of the record
        assert_within_one_ulp(float(total), cpu_norm32([g0, other0]), f"clip n={n} {dtype} offset {off}")
        assert same_bits(rec[1], torch.clamp(0.5 / (rec[0] + 1e-6), max=1.0)) and float(rec[1]) < 1.0
        want_g.mul_(rec[1])
        want_o.mul_(rec[1])
        assert same_bits(g, want_g) and same_bits(other, want_o)
        assert not torch.equal(g.cpu(), g0)
        for b, o, m in ((buf, off, n), (obuf, (off + 2) % 8, CHUNK - 1)):
            assert bool((b[:o] == SENTINEL).all()) and bool((b[o + m:] == SENTINEL).all())


# ------------------------------------------------------------------ the fold
def build(dtype, master, layout, seed):
    """Parameters with gradients on the device in two param groups of different lr, one optimizer."""
    if layout == "sizes":
        sizes = SIZES
    elif layout == "33":
        sizes = [5 + (i % 3) for i in range(_lib.ADAMW_MAX_TENSORS + 1)]
    else:
        sizes = [CHUNK + 11, 5, 0, 2 * CHUNK + 3, 7, 9]
    params, grads = C.make_problem(sizes, 3, seed=seed, p_dtype=dtype, g_dtype=dtype)
    if layout == "mixed":  # fp32 and bf16 parameters in one optimizer, whatever `dtype` is
        for i in (1, 3):
            params[i] = params[i].bfloat16()
            for gs in grads:
                gs[i] = gs[i].bfloat16()
        for i in (0, 4, 5):
            params[i] = params[i].float()
            for gs in grads:
                gs[i] = gs[i].float()
    ps = [p.to(DEV).clone().requires_grad_(True) for p in params]
    half = len(ps) // 2
    opt = P.FusedAdamW([{"params": ps[:half], "lr": 3e-3}, {"params": ps[half:]}], master_weights=master, **HYPER)
    return ps, grads, opt


def set_grads(ps, gs, skip=()):
    for i, (p, g) in enumerate(zip(ps, gs)):
        p.grad = None if i in skip else g.to(DEV)


@pytest.mark.parametrize("dtype, master", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True)])
@pytest.mark.parametrize("alpha", [0.001, 1.0])
@pytest.mark.parametrize("layout", ["sizes", "33", "mixed"])
def test_folded_clip_is_clip_then_step_bit_for_bit(dtype, master, alpha, layout):
    """step(max_grad_norm=c, polyak=...) against clip_grad_norm_(params, c) then step(polyak=...):
    three updates; two param groups with different lr; after the first update one parameter's
    step count is moved ahead (two buckets under one norm); in the mixed layout fp32 and bf16
    parameters, a zero-length one and one without gradient."""
    skip = (5,) if layout == "mixed" else ()
    tg = torch.Generator().manual_seed(101)
    results = []
    for folded in (True, False):
        ps, grads, opt = build(dtype, master, layout, seed=100)
        targets = [(torch.randn(p.shape, generator=tg.manual_seed(101 + i))).to(p.dtype).to(DEV) for i, p in enumerate(ps[:3])]
        sources = [p.data for p in ps[:3]]
        records = []
        for k, gs in enumerate(grads):
            set_grads(ps, gs, skip)
            live = [p for p in ps if p.grad is not None]
            before = [p.grad.clone() for p in live]
            if folded:
                opt.step(max_grad_norm=1.0, polyak=(targets, sources, alpha))
                assert all(same_bits(p.grad, b) for p, b in zip(live, before))  # .grad is left unclipped
                records.append(opt._clip_buffers[0].clone())
                assert same_bits(opt.grad_norm, records[-1][0]) and same_bits(opt.clip_coef, records[-1][1])
                assert opt.grad_norm.shape == () and opt.clip_coef.device == DEV
            else:
                total = P.clip_grad_norm_(ps, 1.0)
                records.append(total._base.clone())
                assert any(not same_bits(p.grad, b) for p, b in zip(live, before))  # the clip was active
                opt.step(polyak=(targets, sources, alpha))
            if k == 0:
                opt.state[ps[0]]["step"] += 3
        torch.cuda.synchronize()
        results.append((ps, opt, targets, records))
    (pa, oa, ta, ra), (pb, ob, tb, rb) = results
    for k, (a, b) in enumerate(zip(ra, rb)):
        assert same_bits(a, b), ("record", k, fields(a), fields(b))
        assert 0.0 < fields(a)["coef"] < 1.0 and fields(a)["nonfinite"] == 0
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert same_bits(a, b), ("p", i)
        sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
        assert set(sa) == set(sb) and bool(sa) == (i not in skip)
        for key in sa:
            assert same_bits(sa[key], sb[key]), (i, key)
    assert float(oa.state[pa[0]]["step"]) == 6.0 and float(oa.state[pa[1]]["step"]) == 3.0
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert same_bits(a, b), ("target", i)
    assert "max_grad_norm" not in repr(oa.state_dict()["param_groups"])


@pytest.mark.parametrize("dtype, master", [(torch.float32, False), (torch.bfloat16, True)])
def test_coefficient_of_one_is_todays_step(dtype, master):
    results = []
    for clipped in (True, False):
        ps, grads, opt = build(dtype, master, "sizes", seed=110)
        for gs in grads[:2]:
            set_grads(ps, gs)
            if clipped:
                opt.step(max_grad_norm=1e9)
                assert float(opt.clip_coef) == 1.0 and float(opt.grad_norm) > 1.0
            else:
                opt.step()
        results.append((ps, opt))
    (pa, oa), (pb, ob) = results
    for a, b in zip(pa, pb):
        assert same_bits(a, b)
        for key in oa.state[a]:
            assert same_bits(oa.state[a][key], ob.state[b][key]), key


def test_functional_form_with_a_record():
    """adamw_step(max_grad_norm=, grad_norm_record=) against clip_grad_norm_ + adamw_step."""
    sizes = [7, CHUNK + 1]
    params, grads = C.make_problem(sizes, 1, seed=120, g_dtype=torch.bfloat16)
    out = []
    for folded in (True, False):
        ps = [p.to(DEV) for p in params]
        gs = [g.to(DEV) for g in grads[0]]
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        kw = dict(step=2, lr=1e-3, betas=C.BETAS, eps=C.EPS, weight_decay=1e-2)
        if folded:
            rec = torch.zeros(8, device=DEV)
            P.adamw_step(ps, gs, ms, vs, max_grad_norm=1.0, grad_norm_record=rec, **kw)
            assert all(torch.equal(g.cpu(), g0) for g, g0 in zip(gs, grads[0]))
        else:
            holders = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
            for h, g in zip(holders, gs):
                h.grad = g
            rec = P.clip_grad_norm_(holders, 1.0)._base
            P.adamw_step(ps, gs, ms, vs, **kw)
        out.append((ps, ms, vs, rec))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert all(same_bits(x, y) for x, y in zip(a, b))
    assert same_bits(out[0][3], out[1][3]) and 0 < fields(out[0][3])["coef"] < 1
    with pytest.raises(ValueError, match="grad_norm_record"):
        P.adamw_step(out[0][0], [g.to(DEV) for g in grads[0]], out[0][1], out[0][2], step=3, lr=1e-3, betas=C.BETAS,
                     eps=C.EPS, weight_decay=0.0, max_grad_norm=1.0, grad_norm_record=torch.zeros(7, device=DEV))


# ------------------------------------------------------------------ ten-step accuracy
def test_ten_step_accuracy_against_the_fp64_oracle():
    """fp32, the cosine schedule of adamw_checks, the clip active on the odd steps and idle on the
    even ones: the folded route and torch's route (clip_grad_norm_ + AdamW on the device) against
    the oracle that clips in fp64; accepted when e_fused <= 2 * e_torch at every step."""
    params, grads = G.make_clip_problem(SIZES, 10, seed=130)
    norms = [G.norm64(gs) for gs in grads]
    c = math.sqrt(norms[0] * norms[1])
    assert all(n > 2 * c for n in norms[0::2]) and all(n < c / 2 for n in norms[1::2])
    wd = HYPER["weight_decay"]
    oracle = G.oracle_run_clipped(params, grads, wd, c)

    def on_device():
        return [p.to(DEV).clone().requires_grad_(True) for p in params]

    torch32 = C.run_optimizer(lambda q: G.ClippedAdamW(q, c, **HYPER), on_device(), grads)
    fused = C.run_optimizer(lambda q: P.FusedAdamW(q, max_grad_norm=c, **HYPER), on_device(), grads)
    figures = []
    for k in range(10):
        e_fused = C.compare(fused[k]["p"], fused[k]["m"], fused[k]["v"], oracle[k])
        e_torch = C.compare(torch32[k]["p"], torch32[k]["m"], torch32[k]["v"], oracle[k])
        print("step", k + 1, "e_fused", e_fused, "e_torch", e_torch)
        figures.append({"step": k + 1, "clipped": k % 2 == 0, "e_fused": e_fused, "e_torch": e_torch})
    path = os.environ.get("TRLX_GRAD_CLIP_PARITY_OUT")
    if path:
        old = json.load(open(path)) if os.path.exists(path) else []
        old.append({"rule": "e_fused <= 2 * e_torch for each of p, m, v (adamw_checks.compare) against the fp64 "
                            "oracle that clips in fp64; torch = clip_grad_norm_ + AdamW in fp32 on the device",
                    "max_norm": c, "sizes": SIZES, "steps": figures})
        with open(path, "w") as f:
            json.dump(old, f, indent=1)
    for rec in figures:
        assert C.accepted(rec["e_fused"], rec["e_torch"]), rec


# ------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient(bad):
    n = CHUNK + 11
    params, grads = C.make_problem([n, 7], 2, seed=140)
    out = []
    for folded in (True, False):
        ps = [p.to(DEV).clone().requires_grad_(True) for p in params]
        opt = P.FusedAdamW(ps, **HYPER)
        set_grads(ps, grads[0])
        opt.step()  # finite state first
        set_grads(ps, grads[1])
        ps[0].grad[4099] = bad
        if folded:
            opt.step(max_grad_norm=1.0)
            rec = opt._clip_buffers[0]
        else:
            rec = take_record([p.grad for p in ps], 1.0)
            for p in ps:
                p.grad.mul_(rec[1])  # torch's multiply by the recorded coefficient
            opt.step()
        out.append((ps, opt, rec))
    f = fields(out[0][2])
    assert same_bits(out[0][2], out[1][2]) and f["nonfinite"] == 1
    if math.isinf(bad):
        assert f["norm"] == math.inf and f["coef"] == 0.0
    else:
        assert math.isnan(f["norm"]) and math.isnan(f["coef"])
    (pa, oa, _), (pb, ob, _) = out
    for a, b in zip(pa, pb):
        assert same_bits(a, b)
        for key in ("exp_avg", "exp_avg_sq"):
            assert same_bits(oa.state[a][key], ob.state[b][key]), key
    # inf: coef 0 zeroes every finite element and inf·0 poisons the one; nan: everything is NaN
    poisoned = torch.isnan(pa[0].detach())
    assert bool(poisoned[4099]) and int(poisoned.sum()) == (1 if math.isinf(bad) else n)
    # error_if_nonfinite raises torch's error and leaves the gradients as they were
    before = [p.grad.clone() for p in pa]
    with pytest.raises(RuntimeError, match="non-finite"):
        P.clip_grad_norm_(pa, 1.0, error_if_nonfinite=True)
    assert all(same_bits(p.grad, b) for p, b in zip(pa, before))
    set_grads(pa, grads[0])
    assert math.isfinite(float(P.clip_grad_norm_(pa, 1.0, error_if_nonfinite=True)))  # finite: no error, clipped
    assert not torch.equal(pa[0].grad.cpu(), grads[0][0])


# ------------------------------------------------------------------ stream, allocation
def test_clipped_step_on_a_side_stream_needs_no_sync_and_no_allocation():
    """Gradients produced on a non-default stream and stepped there with the clip: every launch
    (sumsq, finish, step) is ordered behind its producers on that stream; from the second clipped
    step on, nothing is allocated on the device."""
    n = 4 * CHUNK + 5
    gen = torch.Generator().manual_seed(21)
    a = torch.randn(1024, 1024, generator=gen).to(DEV)
    p0 = torch.randn(n, generator=gen).to(DEV)
    torch.cuda.synchronize()

    def produce_and_step():
        x = a
        for _ in range(20):  # a few hundred microseconds of producer work in front of the step
            x = torch.tanh(x @ a * 1e-2)
        g = x.reshape(-1)[:n].contiguous()
        p = torch.nn.Parameter(p0 + x.reshape(-1)[n:2 * n] * 0)
        p.grad = g
        # the producers' output is tiny; with max_norm <= 1e-7 the coefficient is below 1 whatever the
        # norm (coef <= max_norm / 1e-6)
        opt = P.FusedAdamW([p], lr=1e-3, betas=C.BETAS, weight_decay=1e-2, max_grad_norm=1e-8)
        opt.step()
        allocated = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        opt.step()
        opt.step(max_grad_norm=5e-9)
        assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == allocated
        return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt._clip_buffers[0]

    want = [t.clone() for t in produce_and_step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = produce_and_step()
        host = [t.cpu() for t in got]  # the copy is ordered on the side stream; no device sync
    for w, h in zip(want[:3], host[:3]):
        assert torch.equal(w.cpu(), h)
    # the record: the same norm, coefficient and flag (its fp64 sum depends on the addresses' phase)
    assert torch.equal(want[3].cpu()[:3], host[3][:3])
    assert 0.0 < float(host[3][1]) < 1.0 and bool(host[1].abs().sum() > 0)


# ------------------------------------------------------------------ ILQL heads
def test_ilql_heads_step_and_sync_with_the_clip():
    """ILQLHeads.step_and_sync(opt, max_grad_norm=1.0) leaves what clip_grad_norm_, opt.step() and
    sync_target_q_heads() leave."""
    torch.manual_seed(0)
    cfg = P.ILQLConfig()
    proto = P.ILQLHeads(cfg, 16, 37)
    g = torch.Generator().manual_seed(16)
    grads = {n: torch.randn(p.shape, generator=g) for n, p in proto.named_parameters() if p.requires_grad}
    out = []
    for folded in (True, False):
        heads = copy.deepcopy(proto).to(DEV)
        trainable = [p for p in heads.parameters() if p.requires_grad]
        opt = P.FusedAdamW(trainable, lr=1e-2, betas=C.BETAS)
        for _ in range(2):
            for n, p in heads.named_parameters():
                if p.requires_grad:
                    p.grad = grads[n].to(DEV)
            if folded:
                heads.step_and_sync(opt, max_grad_norm=1.0)
                assert 0.0 < float(opt.clip_coef) < 1.0
            else:
                P.clip_grad_norm_(trainable, 1.0)
                opt.step()
                heads.sync_target_q_heads()
        out.append({k: v.clone() for k, v in heads.state_dict().items()})
    for k in out[0]:
        assert same_bits(out[0][k], out[1][k]), k
        assert not torch.equal(out[0][k].cpu(), proto.state_dict()[k]), k
