"""The bf16-state AdamW chain against torch, and the refusals that need no device.

adamw_bf16_checks.bf16_chain_step is what trlx_adamw_step_ex(state_dtype = TRLX_BF16) computes
per element; this file pins that restatement to torch.optim.AdamW(foreach=False) on bf16 CPU
tensors: 20,000 elements, gradients N(0,1)·10^U{-4..2}, ten updates under CosineAnnealingLR,
betas (0.9, 0.95), weight decay 0.01, every update started from torch's own state.

p and exp_avg_sq must be bit-equal.  exp_avg may differ by one bf16 ulp in at most 1e-3 of the
element-steps, the ulp taken at the larger of the result and the exp_avg the update began from
(adamw_bf16_checks.ulp_report: where g = -9·m the lerp cancels to 0 in one form and to a
residue of 1e-8·m in the other, which no ulp of the result can express): torch's CPU lerp_ evaluates m + w·(g - m) with a fused multiply-add, the kernel
keeps the unfused form that adamw_one already uses for the fp32 state,
    m = bf(add_rn(m, mul_rn(w1, sub_rn(g, m)))),
so the two round differently on a few elements in 10^5.  The fused alternative would be
    m = bf(fma(w1, sub_rn(g, m), m)),
which test_fused_lerp_is_torchs_cpu_form shows to leave no difference at all on this CPU.
"""
import copy

import pytest
import torch

import trlx_t5_amd as P
import adamw_bf16_checks as B
import adamw_checks as C

N, STEPS, WD, SEED = 20000, 10, 0.01, 0


@pytest.fixture(scope="module")
def torch_trajectory():
    """Per update: (step, lr, the bf16 p, g, m, v torch started from, the p, m, v it left)."""
    params, grads = C.make_problem([N], STEPS, seed=SEED, p_dtype=torch.bfloat16, g_dtype=torch.bfloat16)
    p = params[0].clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=C.LR_INIT, betas=C.BETAS, eps=C.EPS, weight_decay=WD, foreach=False)
    out = []
    for k, lr in enumerate(C.cosine_lrs(STEPS), start=1):
        opt.param_groups[0]["lr"] = lr
        p.grad = grads[k - 1][0].clone()
        st = opt.state.get(p, {})
        before = (p.detach().clone(), p.grad.clone(),
                  st["exp_avg"].clone() if st else torch.zeros_like(p.detach()),
                  st["exp_avg_sq"].clone() if st else torch.zeros_like(p.detach()))
        opt.step()
        st = opt.state[p]
        assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.bfloat16  # torch's layout
        out.append((k, lr, before, (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())))
    return out


def test_chain_is_torchs_bf16_adamw(torch_trajectory):
    differ = {"p": 0, "m": 0, "v": 0}
    worst_m = 0.0
    for step, lr, (p, g, m, v), want in torch_trajectory:
        got = B.bf16_chain_step(p, g, m, v, step, lr, C.BETAS, C.EPS, WD)
        for name, a, b in zip("pmv", got, want):
            differ[name] += int((~B.same_bits(a, b)).sum())
        worst_m = max(worst_m, B.ulp_report(got[1], want[1], start=m)[1])
    total = N * STEPS
    print("element-steps", total, "differing", differ, "largest exp_avg difference in bf16 ulps", worst_m)
    assert differ["p"] == 0 and differ["v"] == 0, differ
    assert worst_m <= 1.0, worst_m
    assert differ["m"] <= 1e-3 * total, differ


def test_fused_lerp_is_torchs_cpu_form(torch_trajectory):
    """The form the kernel does NOT take, measured: lerp as one fma (the exact fp32 product and
    sum formed in float64, rounded to fp32, then to bf16) is not further from torch's CPU lerp_
    than the unfused form."""
    fused = unfused = 0
    for step, lr, (p, g, m, v), want in torch_trajectory:
        w1 = torch.tensor(float(B.step_scalars(step, lr, C.BETAS, C.EPS, WD)[1]), dtype=torch.float32)
        gf, mf = g.float(), m.float()
        one_fma = (w1.double() * (gf - mf).double() + mf.double()).float().to(torch.bfloat16)
        two_ops = (mf + w1 * (gf - mf)).to(torch.bfloat16)
        fused += int((~B.same_bits(one_fma, want[1])).sum())
        unfused += int((~B.same_bits(two_ops, want[1])).sum())
    print("exp_avg element-steps differing from torch: fused lerp", fused, "unfused (the kernel's)", unfused)
    assert fused <= unfused


def test_chain_rounding_points():
    """Hand-checked elements: step 1 with g = 0 leaves denom = bf(eps); a large v stands still."""
    bf16 = torch.bfloat16
    p = torch.tensor([1.0, 1.0], dtype=bf16)
    g = torch.tensor([0.0, 1.0], dtype=bf16)
    m, v = torch.zeros(2, dtype=bf16), torch.zeros(2, dtype=bf16)
    p1, m1, v1 = B.bf16_chain_step(p, g, m, v, 1, 1e-3, (0.9, 0.95), 1e-8, 0.0)
    assert float(m1[0]) == 0.0 and float(v1[0]) == 0.0 and float(p1[0]) == 1.0  # 0 / bf(eps) = 0
    assert float(m1[1]) == float(torch.tensor(0.1).to(bf16)) and float(v1[1]) == float(torch.tensor(0.05).to(bf16))
    # v = 1, g = 2^-6: w2·g² = 0.05·2^-12 is far below half an ulp of bf(0.95): v only decays
    v_big = torch.tensor([1.0], dtype=bf16)
    _, _, v2 = B.bf16_chain_step(p[:1], torch.tensor([2.0 ** -6], dtype=bf16), m[:1], v_big, 5, 1e-3, (0.9, 0.95),
                                 1e-8, 0.0)
    assert float(v2) == float(torch.tensor(0.95).to(bf16))
    # beta2 = 0.999 rounds v·b2 back to v for v = 1: bf(0.999) = 1 - 2^-8·... is not representable next to 1
    _, _, v3 = B.bf16_chain_step(p[:1], torch.tensor([2.0 ** -6], dtype=bf16), m[:1], v_big, 5, 1e-3, (0.9, 0.999),
                                 1e-8, 0.0)
    assert float(v3) == 1.0  # the stagnation torch's bf16 AdamW has too


# ------------------------------------------------------------------ refusals without a device
def test_constructor_conflicts():
    w = [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))]
    with pytest.raises(ValueError, match="master_weights"):
        P.FusedAdamW(w, state_dtype="param", master_weights=True)
    with pytest.raises(ValueError, match="state_dtype"):
        P.FusedAdamW(w, state_dtype="bfloat16")
    assert P.FusedAdamW(w).state_dtype == "float32"
    assert P.FusedAdamW(w, state_dtype="param").state_dtype == "param"


def test_param_state_is_zeros_like_the_parameter():
    w = [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(3))]
    opt = P.FusedAdamW(w, state_dtype="param")
    for p in w:
        st = opt._init_state(p)
        assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == p.dtype and "master" not in st
    opt32 = P.FusedAdamW(w)
    assert opt32._init_state(w[0])["exp_avg"].dtype == torch.float32


def test_param_state_refuses_an_fp32_grad_of_a_bf16_parameter():
    w = [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))]
    opt = P.FusedAdamW(w, state_dtype="param")
    if hasattr(w[0], "grad_dtype"):  # newer torch pins .grad to the parameter's dtype unless told otherwise
        w[0].grad_dtype = None
    w[0].grad = torch.zeros(4)
    with pytest.raises(ValueError):  # on a CPU tensor the device check may come first: either is a refusal
        opt.step()


def test_adamw_step_moment_dtypes():
    bf16 = torch.bfloat16
    kw = dict(step=1, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0)
    p, g, m, v = (torch.zeros(6, dtype=bf16) for _ in range(4))
    with pytest.raises(ValueError, match=r"tensor 0: exp_avg_sq must be float32 as exp_avg is"):
        P.adamw_step([p], [g], [m.float()], [v], **kw)
    with pytest.raises(ValueError, match=r"tensor 0: exp_avg must be float32 as exp_avg_sq is"):
        P.adamw_step([p], [g], [m], [v.float()], **kw)
    with pytest.raises(ValueError, match=r"tensor 1: exp_avg is torch.float32 but tensor 0's is torch.bfloat16"):
        P.adamw_step([p, p.clone()], [g, g], [m, m.float()], [v, v.float()], **kw)
    with pytest.raises(ValueError, match=r"tensor 0: bfloat16 exp_avg / exp_avg_sq need a bfloat16 parameter"):
        P.adamw_step([p.float()], [g], [m], [v], **kw)
    with pytest.raises(ValueError, match=r"tensor 0: bfloat16 exp_avg / exp_avg_sq need a bfloat16 parameter"):
        P.adamw_step([p], [g.float()], [m], [v], **kw)
    with pytest.raises(ValueError, match=r"tensor 0: bfloat16 exp_avg / exp_avg_sq take no master"):
        P.adamw_step([p], [g], [m], [v], masters=[p.float()], **kw)
    with pytest.raises(ValueError, match="ROCm"):  # everything valid: only the device is missing
        P.adamw_step([p], [g], [m], [v], **kw)


def test_load_state_dict_under_param_takes_torchs_layout():
    """bf16 moments as saved, fp32 moments rounded to bf16 once, a checkpoint with masters refused."""
    bf16 = torch.bfloat16
    w = [torch.nn.Parameter(torch.zeros(5, dtype=bf16))]
    src = torch.optim.AdamW(w, lr=1e-3)
    m = torch.tensor([1.0, 1.00390625, 1.005859375, -3.0e-5, 0.1], dtype=torch.float32)
    src.state[w[0]] = {"step": torch.tensor(3.0), "exp_avg": m.to(bf16), "exp_avg_sq": (m * m).to(bf16)}
    opt = P.FusedAdamW(w, state_dtype="param")
    opt.load_state_dict(copy.deepcopy(src.state_dict()))
    st = opt.state[w[0]]
    assert st["exp_avg"].dtype == bf16 and torch.equal(st["exp_avg"], m.to(bf16))
    assert torch.equal(st["exp_avg_sq"], (m * m).to(bf16)) and float(st["step"]) == 3.0
    # an fp32-state checkpoint: one rounding (RNE: 1.00390625 = 1 + 2^-8 ties to even, 1.0)
    src32 = P.FusedAdamW(w)
    src32.state[w[0]] = {"step": torch.tensor(3.0), "exp_avg": m.clone(), "exp_avg_sq": m * m}
    opt.load_state_dict(copy.deepcopy(src32.state_dict()))
    st = opt.state[w[0]]
    assert st["exp_avg"].dtype == bf16 and torch.equal(st["exp_avg"], m.to(bf16)) and float(st["exp_avg"][1]) == 1.0
    assert torch.equal(st["exp_avg_sq"], (m * m).to(bf16))
    # and the default keeps widening a torch checkpoint, as before
    opt32 = P.FusedAdamW(w)
    opt32.load_state_dict(copy.deepcopy(src.state_dict()))
    assert opt32.state[w[0]]["exp_avg"].dtype == torch.float32
    sd = copy.deepcopy(src32.state_dict())
    sd["state"][0]["master"] = torch.zeros(5)
    with pytest.raises(ValueError, match="masters"):
        opt.load_state_dict(sd)
