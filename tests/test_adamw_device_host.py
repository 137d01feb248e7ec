"""Host-side checks of the device-resident AdamW schedule (no GPU).

trlx_adamw_sched_scalars_host — the function k_adamw_advance runs on the device, exported for
the host — equals the pure-Python restatement (adamw_device_checks.scalars: a square-and-multiply
product chain in Python floats, numpy.float32 roundings) bit for bit over steps 1..10000.

Measured against the pow() route of the default mode (the same formulas with the C library's
pow): of 10000 steps, 0 round differently in any scalar with betas (0.9, 0.95) and 0 with betas
(0.9, 0.999), over all of lr in {1e-4, 1e-3} x wd in {0, 1e-6, 1e-2} (a step counts when any
combination differs; the test prints the counts).  The two routes do differ in the last places
of the float64 power; a difference of a few 1e-16 survives the rounding to float32 (6e-8) about
once in 1e8 scalars, so none showed in this range.  That count is a measurement, not a tolerance:
the GPU tests compare the two modes bit for bit only on adamw_device_checks.GPU_TUPLES, and this
file asserts that the two routes agree on every step of those tuples.

Also: every refusal of trlx_adamw_advance / trlx_adamw_step_dev / trlx_adamw_step_clipped_dev
with made-up addresses (nothing is launched), the argument errors of FusedAdamW's capturable
mode, schedule_table against a real torch.optim.AdamW + scheduler, the ctypes mirrors.
"""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import adamw_device_checks as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG = 0, 5
BASE = 0x7000_0000_0000  # made-up device addresses: nothing is launched, nothing dereferenced


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "trlx-t5_amd", "csrc"), "-j8"])
    return _lib.load()


def host_scalars(lib, step, lr, b1, b2, eps, wd, alpha):
    out = (ctypes.c_float * 9)()
    assert lib.trlx_adamw_sched_scalars_host(step, lr, b1, b2, eps, wd, alpha, out) == OK
    return np.frombuffer(out, dtype=np.float32).copy()


# ------------------------------------------------------------------ the product chain
@pytest.mark.parametrize("betas", [(0.9, 0.95), (0.9, 0.999)])
def test_host_export_is_the_product_chain_bit_for_bit(lib, betas):
    differs = set()
    for lr in (1e-4, 1e-3):
        for wd in (0.0, 1e-6, 1e-2):
            for step in range(1, 10001):
                got = host_scalars(lib, step, lr, betas[0], betas[1], D.EPS, wd, 0.25)
                want = D.scalars(step, lr, betas[0], betas[1], D.EPS, wd, 0.25)
                assert D.same_bits(got, want), (step, lr, wd, got, want)
                if not D.same_bits(want, D.scalars(step, lr, betas[0], betas[1], D.EPS, wd, 0.25, power=D.pow_libm)):
                    differs.add(step)
    print(f"betas {betas}: {len(differs)} of 10000 steps round differently from the pow route in some scalar")


def test_chain_is_exact_where_it_must_be():
    assert D.pow_chain(0.9, 1) == 0.9 and D.pow_chain(0.5, 10) == 2.0 ** -10 and D.pow_chain(0.9, 0) == 1.0
    assert D.pow_chain(0.9, 3) == (0.9 * (0.9 * 0.9))  # bits 1,1: r = x; x = x*x; r = r*x


def test_host_export_refuses_step_zero_and_null(lib):
    out = (ctypes.c_float * 9)()
    assert lib.trlx_adamw_sched_scalars_host(0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.0, out) == ERR_ARG
    assert lib.trlx_adamw_sched_scalars_host(1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.0, None) == ERR_ARG


@pytest.mark.parametrize("name", sorted(D.GPU_TUPLES))
def test_both_routes_agree_on_every_tuple_the_gpu_tests_use(lib, name):
    (b1, b2), rates, wd, alpha, first = D.GPU_TUPLES[name]
    for k, lr in enumerate(rates):
        step = first + k
        chain = D.scalars(step, lr, b1, b2, D.EPS, wd, alpha)
        assert D.same_bits(chain, D.scalars(step, lr, b1, b2, D.EPS, wd, alpha, power=D.pow_libm)), (name, step)
        assert D.same_bits(chain, host_scalars(lib, step, lr, b1, b2, D.EPS, wd, alpha)), (name, step)


# ------------------------------------------------------------------ schedule_table
def test_schedule_table_is_torchs_schedule():
    p = torch.zeros(3, requires_grad=True)
    opt = torch.optim.AdamW([p], lr=D.LR_INIT)
    sched = D.cosine(opt)
    seen = []
    for _ in range(12):
        seen.append(opt.param_groups[0]["lr"])
        p.grad = torch.ones(3)
        opt.step()
        sched.step()
    table = P.schedule_table(D.cosine, 12, D.LR_INIT)
    assert table.dtype == torch.float64 and table.tolist() == seen == D.GPU_TUPLES["cosine12"][1]
    with pytest.raises(ValueError):
        P.schedule_table(D.cosine, 0, D.LR_INIT)


# ------------------------------------------------------------------ argument errors of the Python layer
def params(n=2):
    return [torch.zeros(4, requires_grad=True) for _ in range(n)]


@pytest.mark.parametrize("kw", [dict(skip_nonfinite=True), dict(sync_every=3), dict(lr_schedule=[1e-3])])
def test_device_decisions_need_capturable(kw):
    with pytest.raises(ValueError, match="capturable"):
        P.FusedAdamW(params(), **kw)
    P.FusedAdamW(params(), capturable=True, **kw)  # accepted; nothing touches a device before step()


@pytest.mark.parametrize("bad", [-1, 1.5])
def test_sync_every_must_be_a_count(bad):
    with pytest.raises(ValueError, match="sync_every"):
        P.FusedAdamW(params(), capturable=True, sync_every=bad)


def test_default_mode_is_unchanged_and_has_no_device_views():
    opt = P.FusedAdamW(params())
    assert opt.capturable is False and opt.applied_steps is None and opt.defaults["capturable"] is False
    assert P.FusedAdamW(params(), capturable=True).defaults["capturable"] is True


def test_a_missing_gradient_is_refused_in_capturable_mode():
    ps = params()
    ps[0].grad = torch.ones(4)
    opt = P.FusedAdamW(ps, capturable=True)
    with pytest.raises(ValueError, match="no gradient"):
        opt.step()
    assert len(opt.state) == 0


def test_a_polyak_source_outside_the_step_is_refused_with_a_cadence():
    ps = params()
    for p in ps:
        p.grad = torch.ones(4)
    opt = P.FusedAdamW(ps, capturable=True, sync_every=3)
    outside, target = torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError, match="sync_every"):
        opt.step(polyak=([target], [outside], 0.5))
    assert len(opt.state) == 0


@pytest.mark.parametrize("sch", [[], [float("nan")], [-1.0], [float("inf")], [[1e-3], []], [1e-3, [1e-4]], "fast",
                                 torch.zeros(2, 2, 2), torch.zeros(0)])
def test_bad_schedules_are_refused_by_the_constructor(sch):
    with pytest.raises(ValueError, match="lr_schedule"):
        P.FusedAdamW(params(), capturable=True, lr_schedule=sch)


def test_the_number_of_tables_must_be_the_number_of_groups():
    a, b = params(1), params(1)
    for sch in ([[1e-3], [1e-4]], torch.full((2, 3), 1e-3)):
        with pytest.raises(ValueError, match="param groups"):
            P.FusedAdamW(a, capturable=True, lr_schedule=sch)  # two tables, one group
        opt = P.FusedAdamW([{"params": a}, {"params": b}], capturable=True, lr_schedule=sch)
        assert opt._group_rates(1).tolist() == [float(x) for x in sch[1]]
        opt.add_param_group({"params": params(1)})
        with pytest.raises(ValueError, match="param groups"):
            opt._group_rates(2)


def test_a_flat_list_of_zero_dim_tensors_is_one_table():
    opt = P.FusedAdamW([{"params": params(1)}, {"params": params(1)}], capturable=True,
                       lr_schedule=[torch.tensor(1e-3), torch.tensor(5e-4, dtype=torch.float64)])
    assert opt._group_rates(0).tolist() == opt._group_rates(1).tolist() == [float(torch.tensor(1e-3)), 5e-4]


def test_a_polyak_source_outside_the_step_is_refused_with_the_skip():
    ps = params()
    for p in ps:
        p.grad = torch.ones(4)
    opt = P.FusedAdamW(ps, capturable=True, skip_nonfinite=True)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        opt.step(polyak=([torch.zeros(4)], [torch.zeros(4)], 0.5))
    assert len(opt.state) == 0


def test_load_state_dict_needs_one_step_per_group():
    ps = params()
    donor = torch.optim.AdamW(ps, lr=1e-3)
    for p in ps:
        p.grad = torch.ones(4)
    donor.step()
    sd = copy.deepcopy(donor.state_dict())
    opt = P.FusedAdamW(ps, capturable=True)
    opt.load_state_dict(copy.deepcopy(sd))  # agreeing CPU steps load (the record is written on the device later)
    assert opt._pending_step == {0: 1} and opt.param_groups[0]["capturable"] is True
    sd["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="disagree"):
        P.FusedAdamW(ps, capturable=True).load_state_dict(sd)


# ------------------------------------------------------------------ C-ABI refusals, nothing launched
def advance_call(lib, **over):
    a = _lib.AdamwAdvanceArgs()
    a.sched, a.lr_table, a.n_lr, a.sync_every = BASE, BASE + 4096, 4, 0
    a.beta1, a.beta2, a.eps, a.weight_decay, a.alpha = 0.9, 0.95, 1e-8, 1e-2, 0.5
    a.grad_record, a.skip_nonfinite = BASE + 8192, 1
    for k, v in over.items():
        setattr(a, k, v)
    rc = lib.trlx_adamw_advance(ctypes.byref(a), None)
    return rc, lib.trlx_last_error().decode()


@pytest.mark.parametrize("over, word", [
    (dict(sched=None), "NULL schedule record"), (dict(sched=BASE + 4), "not aligned to 8"),
    (dict(lr_table=None), "NULL lr_table"), (dict(lr_table=BASE + 4100), "lr_table is not aligned"),
    (dict(n_lr=0), "n_lr 0"), (dict(n_lr=-3), "n_lr -3"), (dict(sync_every=-1), "sync_every -1"),
    (dict(beta1=float("nan")), "NaN"), (dict(beta2=float("nan")), "NaN"), (dict(eps=float("nan")), "NaN"),
    (dict(weight_decay=float("nan")), "NaN"), (dict(alpha=float("nan")), "NaN"),
    (dict(grad_record=BASE + 8196), "grad-norm record is not aligned"),
    (dict(lr_table=BASE + 88), "overlaps the lr_table"), (dict(lr_table=BASE - 8), "overlaps the lr_table"),
    (dict(grad_record=BASE + 64), "overlaps the grad-norm record"),
    (dict(grad_record=BASE + 4096 + 24), "lr_table overlaps the grad-norm record")])
def test_advance_refusals(lib, over, word):
    rc, msg = advance_call(lib, **over)
    assert rc == ERR_ARG and word in msg, msg


def test_advance_refuses_null_args(lib):
    assert lib.trlx_adamw_advance(None, None) == ERR_ARG


def step_dev_call(lib, sched, record=None, clipped=False, n=100, target=None, lr_table=None, n_lr=0):
    stride = 1 << 20
    a = _lib.AdamwArgs()
    a.p_dtype, a.g_dtype, a.count = _lib.F32, _lib.F32, 1
    cols = [(ctypes.c_void_p * 1)(v) for v in (BASE, BASE + stride, BASE + 2 * stride, BASE + 3 * stride, None, target)]
    a.p, a.g, a.m, a.v, a.master, a.target = cols
    a.numel = (ctypes.c_int64 * 1)(n)
    a.step, a.lr, a.beta1 = -7, float("nan"), float("nan")  # ignored by the _dev entries
    a.lr_table, a.n_lr = lr_table, n_lr
    if clipped:
        rc = lib.trlx_adamw_step_clipped_dev(ctypes.byref(a), record, sched, None)
    else:
        rc = lib.trlx_adamw_step_dev(ctypes.byref(a), sched, None)
    return rc, lib.trlx_last_error().decode()


FAR = BASE + (64 << 20)


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("sched, word", [
    (None, "NULL schedule record"), (FAR + 4, "schedule record is not aligned"),
    (BASE + 8, "schedule record overlaps p"), (BASE + (1 << 20) - 8, "schedule record overlaps g"),
    (BASE + (2 << 20) + 392, "schedule record overlaps m"), (BASE + (3 << 20), "schedule record overlaps v")])
def test_step_dev_refusals(lib, clipped, sched, word):
    rc, msg = step_dev_call(lib, sched, record=FAR + 4096, clipped=clipped)
    assert rc == ERR_ARG and word in msg, msg


def test_step_dev_refuses_a_schedule_record_on_the_target_or_the_clip_record(lib):
    rc, msg = step_dev_call(lib, BASE + (5 << 20), target=BASE + (5 << 20) + 16)
    assert rc == ERR_ARG and "schedule record overlaps target" in msg
    rc, msg = step_dev_call(lib, FAR, record=FAR + 88, clipped=True)
    assert rc == ERR_ARG and "overlaps the clip record" in msg
    rc, msg = step_dev_call(lib, FAR, record=None, clipped=True)
    assert rc == ERR_ARG and "NULL grad-norm record" in msg
    assert lib.trlx_adamw_step_dev(None, FAR, None) == ERR_ARG


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("lr_table, n_lr, word", [
    (BASE + 16, 4, "lr_table overlaps p"), (BASE + (1 << 20) - 8, 2, "lr_table overlaps g"),
    (BASE + (2 << 20) + 392, 1, "lr_table overlaps m"), (BASE + (3 << 20) - 800, 101, "lr_table overlaps v"),
    (FAR + 8192 + 4, 4, "lr_table is not aligned"), (FAR + 8192, 0, "n_lr 0"), (FAR + 8192, -2, "n_lr -2"),
    (FAR + 88, 4, "schedule record overlaps the lr_table"), (FAR - 16, 3, "schedule record overlaps the lr_table")])
def test_step_dev_refuses_an_lr_table_on_its_tensors(lib, clipped, lr_table, n_lr, word):
    rc, msg = step_dev_call(lib, FAR, record=FAR + 4096, clipped=clipped, lr_table=lr_table, n_lr=n_lr)
    assert rc == ERR_ARG and word in msg, msg


def test_step_dev_refuses_an_lr_table_on_the_target_or_the_clip_record(lib):
    rc, msg = step_dev_call(lib, FAR, target=BASE + (5 << 20), lr_table=BASE + (5 << 20) + 8, n_lr=1)
    assert rc == ERR_ARG and "lr_table overlaps target" in msg
    rc, msg = step_dev_call(lib, FAR, record=FAR + 4096, clipped=True, lr_table=FAR + 4096 + 24, n_lr=5)
    assert rc == ERR_ARG and "lr_table overlaps the clip record" in msg


def test_the_host_scalar_entries_never_read_the_lr_table(lib):
    """trlx_adamw_step with a misaligned lr_table on its own parameter: the fields belong to the
    _dev entries; with nothing live to launch the call succeeds without a device."""
    a = _lib.AdamwArgs()
    a.p_dtype, a.g_dtype, a.count = _lib.F32, _lib.F32, 0
    a.step, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = 1, 1e-3, 0.9, 0.95, 1e-8, 0.0
    a.lr_table, a.n_lr = BASE + 3, -1
    assert lib.trlx_adamw_step(ctypes.byref(a), None) == OK


def test_step_dev_ignores_the_scalar_fields_and_accepts_an_empty_list(lib):
    """step = -7 and NaN hyper-parameters are not validated by the _dev entries: with nothing
    live to launch (numel 0) the call succeeds without a device."""
    rc, msg = step_dev_call(lib, FAR, n=0)
    assert rc == OK, msg
    rc, msg = step_dev_call(lib, FAR, record=FAR + 4096, clipped=True, n=0)
    assert rc == OK, msg


# ------------------------------------------------------------------ mirrors
@pytest.mark.parametrize("cname, mirror", [("trlx_adamw_sched", _lib.AdamwSched),
                                           ("trlx_adamw_advance_args", _lib.AdamwAdvanceArgs)])
def test_mirror_layout_matches_header(tmp_path, cname, mirror):
    fields = [f[0] for f in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof({cname}, {f}));\n' for f in fields)
                   + f'printf("%zu\\n", sizeof({cname}));\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [getattr(mirror, f).offset for f in fields] + [ctypes.sizeof(mirror)]
    if cname == "trlx_adamw_sched":
        assert ctypes.sizeof(mirror) == 96 and mirror.decay.offset == 24 and mirror.lr.offset == 64
