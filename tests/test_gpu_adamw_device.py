"""FusedAdamW(capturable=True) on the GPU: step counter, learning rate, non-finite skip and sync
cadence on the device (trlx_adamw_advance, trlx_adamw_step_dev, trlx_adamw_step_clipped_dev).

No tolerance anywhere: the capturable mode is compared bit for bit (torch.equal) with the
default mode driven by the real torch scheduler, on the step ranges of
adamw_device_checks.GPU_TUPLES, where the product chain and pow() give the same scalars (the CPU
suite asserts that).

Geometry (that of test_gpu_adamw.py): tensors of 1, 7, chunk - 1, chunk, chunk + 1 elements, an
empty one, parameters and gradients as views at element offsets 1 and 3 (the element path; the
others take the vector path), 33 live tensors (two launches).
"""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
from trlx_t5_amd import optim as O
import adamw_device_checks as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = _lib.ADAMW_CHUNK
SIZES = [1, 7, CHUNK - 1, CHUNK, CHUNK + 1, 0]
VIEWS = [(CHUNK + 1, 1), (7, 3)]           # (numel, element offset) of misaligned parameter / gradient views
SMALL = [5 + (i % 3) for i in range(26)]   # 5 + 2 + 26 = 33 live tensors: one more than a table
GUARD = 768.0  # exact in bfloat16
PAIRS = {"fp32": (torch.float32, torch.float32, False), "bf16": (torch.bfloat16, torch.bfloat16, False),
         "bf16_master": (torch.bfloat16, torch.bfloat16, True), "bf16_p_fp32_g": (torch.bfloat16, torch.float32, False)}


def layout(sizes=SIZES, views=VIEWS, small=SMALL):
    return [(n, 0) for n in sizes] + list(views) + [(n, 0) for n in small]


def problem(shape, steps, seed, p_dtype, g_dtype):
    """CPU values: parameters and per-step gradients for a layout of (numel, offset)."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g).to(p_dtype) for n, _ in shape]
    gs = [[(torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 2, (1,), generator=g))).to(g_dtype)
           for n, _ in shape] for _ in range(steps)]
    return ps, gs


def placed(t, off):
    """`t` on the device as a view at element `off` of a guard-filled buffer: (buffer, view)."""
    buf = torch.full((t.numel() + off + 8,), GUARD, dtype=t.dtype, device=DEV)
    view = buf[off:off + t.numel()]
    view.copy_(t)
    return buf, view


def leaves(ps, shape):
    bufs, views = zip(*[placed(p, off) for p, (_, off) in zip(ps, shape)])
    params = [v.detach().requires_grad_(True) for v in views]
    for p in params:
        if hasattr(p, "grad_dtype"):
            p.grad_dtype = None  # a bf16 parameter may carry an fp32 gradient
    return bufs, params


def set_grads(params, grads, shape, static=None):
    for i, (p, g, (_, off)) in enumerate(zip(params, grads, shape)):
        if static is not None:
            static[i].copy_(g)
            p.grad = static[i]
        else:
            p.grad = placed(g, off)[1]


def snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state[p]
        out.append([p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
                   + ([st["master"].clone()] if "master" in st else []))
    return out


def same(a, b):
    return all(torch.equal(x, y) for ta, tb in zip(a, b) for x, y in zip(ta, tb)) and len(a) == len(b)


def guards_intact(bufs, shape):
    return all(bool((b[:off] == GUARD).all()) and bool((b[off + n:] == GUARD).all()) for b, (n, off) in zip(bufs, shape))


def fused(params, **kw):
    kw.setdefault("lr", D.LR_INIT)
    return P.FusedAdamW(params, betas=D.BETAS, eps=D.EPS, weight_decay=D.WEIGHT_DECAY, **kw)


# ------------------------------------------------------------------ bit equality with the host route
@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_twelve_updates_equal_the_host_route_bit_for_bit(pair, max_grad_norm):
    p_dtype, g_dtype, master = PAIRS[pair]
    shape = layout()
    ps, gs = problem(shape, D.N_UPDATES, 21, p_dtype, g_dtype)
    table = P.schedule_table(D.cosine, D.N_UPDATES, D.LR_INIT)
    assert table.tolist() == D.GPU_TUPLES["cosine12"][1]

    _, host_params = leaves(ps, shape)
    host = fused(host_params, master_weights=master, max_grad_norm=max_grad_norm)
    sched = D.cosine(host)
    bufs, dev_params = leaves(ps, shape)
    dev = fused(dev_params, master_weights=master, max_grad_norm=max_grad_norm, capturable=True, lr_schedule=table)
    for k in range(D.N_UPDATES):
        set_grads(host_params, gs[k], shape)
        host.step()
        sched.step()
        set_grads(dev_params, gs[k], shape)
        dev.step()
    assert same(snapshot(dev, dev_params), snapshot(host, host_params))
    assert guards_intact(bufs, shape)
    assert int(dev.applied_steps) == D.N_UPDATES and int(dev.skipped_steps) == 0
    assert float(dev.last_lr) == table[-1].item()
    st = dev.state[dev_params[0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} | ({"master"} if master else set())
    assert st["step"].is_cuda and st["step"].dim() == 0 and int(st["step"]) == D.N_UPDATES
    if max_grad_norm is not None:
        assert torch.equal(dev.grad_norm, host.grad_norm) and torch.equal(dev.clip_coef, host.clip_coef)


def test_the_last_table_entry_holds_and_group_lr_is_followed():
    """A 3-entry table over 5 updates equals the host route at rates [a, b, c, c, c]; with no
    table a changed group['lr'] reaches the device on the next call."""
    shape = layout(sizes=[7, CHUNK + 1], views=[], small=[])
    ps, gs = problem(shape, 5, 22, torch.float32, torch.float32)
    held = D.GPU_TUPLES["table3of5"][1]
    rates = held[:3]
    assert held == rates + [rates[2]] * 2
    runs = {}
    for name, kw in (("host", {}), ("table", dict(capturable=True, lr_schedule=rates)), ("group", dict(capturable=True))):
        _, params = leaves(ps, shape)
        opt = fused(params, **kw)
        for k in range(5):
            if name != "table":
                opt.param_groups[0]["lr"] = rates[min(k, 2)]
            set_grads(params, gs[k], shape)
            opt.step()
        runs[name] = snapshot(opt, params)
        if name != "host":
            assert float(opt.last_lr) == rates[2] and int(opt.applied_steps) == 5
    assert same(runs["table"], runs["host"]) and same(runs["group"], runs["host"])


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("pair", ["fp32", "bf16_master"])
def test_dev_entry_on_views_of_one_phase_takes_the_vector_path_with_a_head(pair, off):
    """p, g, m, v, master, target all at element offset `off`: a shared 16-byte phase, so the
    vector path with a head and a tail.  One advance + trlx_adamw_step_clipped_dev against
    trlx_adamw_step_clipped of the same step number and rate, through the same Python launcher."""
    p_dtype, g_dtype, master = PAIRS[pair]
    (_, _), (lr,), _, alpha, step = D.GPU_TUPLES["phase_step3"]
    n = CHUNK + 11
    assert (step, alpha) == (3, 0.25)
    g = torch.Generator().manual_seed(23)
    base = [torch.randn(n, generator=g).to(p_dtype), torch.randn(n, generator=g).to(g_dtype),
            torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01,
            torch.randn(n, generator=g), torch.randn(n, generator=g).to(p_dtype)]
    record = torch.zeros(O.RECORD_FLOATS, device=DEV)
    grad = base[1].to(DEV)
    O._grad_norm([grad], 1.0, record, torch.empty(8, dtype=torch.float64, device=DEV), 0)

    def run(sched):
        bufs, views = zip(*[placed(t, off) for t in base])
        p, gr, m, v, w, tgt = views
        entry = (p, gr, m, v, w if master else None, tgt)
        O._launch([entry], step, lr, *D.BETAS, D.EPS, D.WEIGHT_DECAY, 0.25, record, sched=sched)
        torch.cuda.synchronize()
        assert all(bool((b[:off] == GUARD).all()) and bool((b[off + n:] == GUARD).all()) for b in bufs)
        return [x.clone() for x in views]

    sched = torch.zeros(O.SCHED_WORDS, dtype=torch.int64, device=DEV)
    sched[0] = step - 1
    a = _lib.AdamwAdvanceArgs()
    table = torch.tensor([lr], dtype=torch.float64, device=DEV)
    a.sched, a.lr_table, a.n_lr, a.sync_every = sched.data_ptr(), table.data_ptr(), 1, 1
    a.beta1, a.beta2, a.eps, a.weight_decay, a.alpha = *D.BETAS, D.EPS, D.WEIGHT_DECAY, 0.25
    _lib.call("trlx_adamw_advance", ctypes.byref(a), _lib.stream_of(sched))
    want, got = run(None), run(sched)
    assert all(torch.equal(x, y) for x, y in zip(want, got))
    assert not torch.equal(got[0].cpu(), base[0]) and not torch.equal(got[5].cpu(), base[5])
    host = D.scalars(step, lr, *D.BETAS, D.EPS, D.WEIGHT_DECAY, 0.25)
    on_device = sched.view(torch.float32)[6:15].cpu().numpy()
    assert D.same_bits(on_device, host), (on_device, host)
    assert sched[:2].tolist() == [step, 0] and sched.view(torch.int32)[4:6].tolist() == [1, 1]


# ------------------------------------------------------------------ non-finite skip
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("pair", ["fp32", "bf16_master"])
def test_a_nonfinite_gradient_skips_the_update_on_the_device(pair, bad):
    p_dtype, g_dtype, master = PAIRS[pair]
    shape = layout(sizes=[7, CHUNK + 1], views=[(9, 1)], small=[])
    ps, gs = problem(shape, 6, 24, p_dtype, g_dtype)
    gs[2][1][CHUNK // 2] = bad  # update 3 of 6
    rates = D.GPU_TUPLES["cosine12"][1][:6]
    tg0 = [torch.randn(n, generator=torch.Generator().manual_seed(25 + i)).to(p_dtype) for i, (n, _) in enumerate(shape)]

    def run(grads, **kw):
        bufs, params = leaves(ps, shape)
        tbufs, targets = zip(*[placed(t, off) for t, (_, off) in zip(tg0, shape)])
        opt = fused(params, master_weights=master, max_grad_norm=1.0, capturable=True, lr_schedule=rates, **kw)
        states, seen = [], []
        for g in grads:
            set_grads(params, g, shape)
            opt.step(polyak=(list(targets), [p.data for p in params], 0.25))
            states.append(snapshot(opt, params) + [[t.clone() for t in targets]])
            seen.append((int(opt.applied_steps), int(opt.skipped_steps)))
        assert guards_intact(bufs, shape) and guards_intact(tbufs, shape)
        return opt, states, seen

    opt, states, counters = run(gs, skip_nonfinite=True)
    assert same(states[2], states[1]) and not same(states[1], states[0])  # update 3 wrote nothing
    assert counters[1] == (2, 0) and counters[2] == (2, 1), counters  # read right after updates 2 and 3
    assert int(opt.applied_steps) == 5 and int(opt.skipped_steps) == 1
    ref, ref_states, _ = run(gs[:2] + gs[3:], skip_nonfinite=True)
    assert same(states[-1], ref_states[-1])  # bias correction and the lr index did not advance
    assert int(ref.applied_steps) == 5 and int(ref.skipped_steps) == 0 and float(opt.last_lr) == rates[4]
    assert all(bool(torch.isfinite(x.float()).all()) for t in states[-1] for x in t)

    # today's behaviour, pinned.  A NaN norm gives a NaN coefficient: every gradient, hence every
    # parameter and moment, becomes NaN.  An inf norm gives coef = 1 / (inf + 1e-6) = 0: the inf
    # element's gradient is inf * 0 = NaN, so that element of p, m and v is lost.
    nan_opt, nan_states, _ = run(gs[:3], skip_nonfinite=False)
    assert int(nan_opt.applied_steps) == 3 and int(nan_opt.skipped_steps) == 0
    hit = nan_states[-1][1]
    assert all(bool(torch.isnan(x[CHUNK // 2].float())) for x in hit[:3])
    if bad != bad:
        for t in nan_states[-1][:-1]:
            assert bool(torch.isnan(t[0].float()).all()) and bool(torch.isnan(t[1]).all())


def test_skip_without_a_clip_still_takes_the_norm():
    shape = layout(sizes=[7, CHUNK + 1], views=[], small=[])
    ps, gs = problem(shape, 3, 26, torch.float32, torch.float32)
    gs[1][0][3] = float("inf")
    runs = {}
    for name, grads, kw in (("skip", gs, dict(skip_nonfinite=True)), ("plain", [gs[0], gs[2]], {})):
        _, params = leaves(ps, shape)
        opt = fused(params, capturable=True, **kw)
        for g in grads:
            set_grads(params, g, shape)
            opt.step()
        runs[name] = snapshot(opt, params)
    assert same(runs["skip"], runs["plain"]) and int(opt.applied_steps) == 2


# ------------------------------------------------------------------ sync cadence
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sync_every_three_over_seven_updates(dtype):
    (b1, b2), rates, wd, alpha, _ = D.GPU_TUPLES["constant7"]
    shape = layout(sizes=[7, CHUNK + 1], views=[(CHUNK + 1, 1)], small=[])
    ps, gs = problem(shape, 7, 27, dtype, dtype)
    tg0 = [torch.randn(n, generator=torch.Generator().manual_seed(28 + i)).to(dtype) for i, (n, _) in enumerate(shape)]

    _, host_params = leaves(ps, shape)
    _, host_targets = zip(*[placed(t, off) for t, (_, off) in zip(tg0, shape)])
    host = fused(host_params, lr=rates[0])
    bufs, dev_params = leaves(ps, shape)
    tbufs, dev_targets = zip(*[placed(t, off) for t, (_, off) in zip(tg0, shape)])
    dev = fused(dev_params, lr=rates[0], capturable=True, sync_every=3)
    for k in range(1, 8):
        set_grads(host_params, gs[k - 1], shape)
        host.step()
        if k % 3 == 0:
            P.polyak_update(list(host_targets), [p.data for p in host_params], alpha)
        before = [t.clone() for t in dev_targets]
        set_grads(dev_params, gs[k - 1], shape)
        dev.step(polyak=(list(dev_targets), [p.data for p in dev_params], alpha))
        assert all(torch.equal(a, b) for a, b in zip(dev_targets, host_targets)), k
        unchanged = all(torch.equal(a, b) for a, b in zip(dev_targets, before))
        assert unchanged == (k % 3 != 0), k
    assert same(snapshot(dev, dev_params), snapshot(host, host_params))
    assert guards_intact(bufs, shape) and guards_intact(tbufs, shape)
    assert dev._sched[0]["record"].view(torch.int32)[4:6].tolist() == [1, 0]  # update 7: applied, no sync


# ------------------------------------------------------------------ no host dependence
def test_reading_the_counter_after_every_step_changes_nothing():
    shape = layout(small=SMALL[:3])
    ps, gs = problem(shape, D.N_UPDATES, 29, torch.float32, torch.float32)
    table = P.schedule_table(D.cosine, D.N_UPDATES, D.LR_INIT)
    runs = []
    for read in (False, True):
        _, params = leaves(ps, shape)
        opt = fused(params, capturable=True, lr_schedule=table, max_grad_norm=1.0)
        grads = [[placed(g, off)[1] for g, (_, off) in zip(step, shape)] for step in gs]  # staged before the loop
        for k in range(D.N_UPDATES):
            for p, g in zip(params, grads[k]):
                p.grad = g
            opt.step()
            if read:
                assert opt.applied_steps.item() == k + 1
        runs.append(snapshot(opt, params))
    assert same(runs[0], runs[1])


def test_state_dict_round_trip_keeps_the_counter():
    shape = layout(sizes=[7, CHUNK + 1], views=[], small=[])
    ps, gs = problem(shape, 4, 30, torch.float32, torch.float32)
    table = D.GPU_TUPLES["cosine12"][1][:4]
    _, params = leaves(ps, shape)
    straight = fused(params, capturable=True, lr_schedule=table)
    for g in gs:
        set_grads(params, g, shape)
        straight.step()
    _, params2 = leaves(ps, shape)
    first = fused(params2, capturable=True, lr_schedule=table)
    for g in gs[:2]:
        set_grads(params2, g, shape)
        first.step()
    sd = first.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    for step_on in ("cuda", "cpu"):
        _, params3 = leaves([p.detach().cpu() for p in params2], shape)
        second = fused(params3, capturable=True, lr_schedule=table)
        loaded = {"state": {k: {n: (t.to(step_on).clone() if n == "step" else t.clone()) for n, t in v.items()}
                            for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]}
        second.load_state_dict(loaded)
        assert int(second.applied_steps) == 2
        for g in gs[2:]:
            set_grads(params3, g, shape)
            second.step()
        assert same(snapshot(second, params3), snapshot(straight, params))
        assert second.state[params3[0]]["step"].is_cuda and int(second.state[params3[0]]["step"]) == 4


# ------------------------------------------------------------------ graph replay
@pytest.mark.timeout(300)
def test_one_captured_update_replays_with_a_moving_counter_and_rate():
    shape = [(7, 0), (CHUNK + 1, 0), (33, 0)]
    ps, gs = problem(shape, 7, 31, torch.float32, torch.float32)
    table = D.GPU_TUPLES["cosine12"][1][:7]

    _, eager_params = leaves(ps, shape)
    eager = fused(eager_params, capturable=True, lr_schedule=table, max_grad_norm=1.0)
    for g in gs:
        set_grads(eager_params, g, shape)
        eager.step()

    _, params = leaves(ps, shape)
    opt = fused(params, capturable=True, lr_schedule=table, max_grad_norm=1.0)
    static = [torch.zeros(n, device=DEV) for n, _ in shape]
    set_grads(params, gs[0], shape, static)
    opt.step()  # warm-up: every buffer exists before the capture
    torch.cuda.synchronize()
    # Is capture available at all?  Decided on a torch op of a scratch tensor, before any of the
    # project's code runs under capture: only that may skip.
    scratch = torch.zeros(8, device=DEV)
    try:
        probe = torch.cuda.CUDAGraph()
        with torch.cuda.graph(probe):
            scratch.add_(1.0)
        probe.replay()
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.skip(f"graph capture is unavailable here: {e}")
    assert scratch.tolist() == [1.0] * 8
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, a linear chain of launches; a failure here fails the test
        opt.step()
    assert int(opt.applied_steps) == 1  # a capture runs nothing
    for g in gs[1:]:
        for buf, new in zip(static, g):
            buf.copy_(new)
        graph.replay()
    torch.cuda.synchronize()
    assert int(opt.applied_steps) == 6 + 1 and float(opt.last_lr) == table[6]
    assert same(snapshot(opt, params), snapshot(eager, eager_params))


# ------------------------------------------------------------------ C-ABI refusals with live tensors
def test_refusals_launch_nothing():
    n = 64
    tensors = [torch.full((n,), GUARD, device=DEV) for _ in range(4)]  # p, g, m, v
    sched = torch.full((O.SCHED_WORDS + 1,), 5, dtype=torch.int64, device=DEV)
    table = torch.full((4,), 0.5, dtype=torch.float64, device=DEV)
    record = torch.zeros(O.RECORD_FLOATS + 2, device=DEV)

    def advance(**over):
        a = _lib.AdamwAdvanceArgs()
        a.sched, a.lr_table, a.n_lr, a.sync_every = sched.data_ptr(), table.data_ptr(), 4, 0
        a.beta1, a.beta2, a.eps, a.weight_decay, a.alpha = *D.BETAS, D.EPS, D.WEIGHT_DECAY, 0.5
        a.grad_record, a.skip_nonfinite = record.data_ptr(), 1
        for k, v in over.items():
            setattr(a, k, v)
        _lib.call("trlx_adamw_advance", ctypes.byref(a), _lib.stream_of(sched))

    def step_dev(sched_ptr, clipped, lr_table=None):
        a = _lib.AdamwArgs()
        a.lr_table, a.n_lr = lr_table, 4
        a.p_dtype, a.g_dtype, a.count = _lib.F32, _lib.F32, 1
        a.p, a.g, a.m, a.v = [(ctypes.c_void_p * 1)(t.data_ptr()) for t in tensors]
        a.numel = (ctypes.c_int64 * 1)(n)
        if clipped:
            _lib.call("trlx_adamw_step_clipped_dev", ctypes.byref(a), record.data_ptr(), sched_ptr, _lib.stream_of(sched))
        else:
            _lib.call("trlx_adamw_step_dev", ctypes.byref(a), sched_ptr, _lib.stream_of(sched))

    for over in (dict(sched=None), dict(sched=sched.data_ptr() + 4), dict(n_lr=0), dict(sync_every=-1),
                 dict(lr_table=sched.data_ptr() + 8), dict(grad_record=sched.data_ptr() + 16),
                 dict(weight_decay=float("nan"))):
        with pytest.raises(ValueError):
            advance(**over)
    for clipped in (False, True):
        for ptr in (None, sched.data_ptr() + 4, tensors[0].data_ptr() + 8, tensors[3].data_ptr(),
                    *([record.data_ptr() + 8] if clipped else [])):
            with pytest.raises(ValueError):
                step_dev(ptr, clipped)
        for lr_table in (tensors[1].data_ptr() + 8, tensors[2].data_ptr() - 8, sched.data_ptr() + 32,
                         table.data_ptr() + 4):
            with pytest.raises(ValueError):
                step_dev(sched.data_ptr(), clipped, lr_table)
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in tensors) and bool((sched == 5).all())
    assert bool((table == 0.5).all()) and bool((record == 0).all())
