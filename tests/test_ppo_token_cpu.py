"""Host-side checks of the [B, T] PPO token kernels (no GPU): the float64 restatements of
ppo_token_checks reproduce the reference's fp32 fixtures; the tie generator plants what it claims;
the GAE launch geometry keeps dynamic + static LDS within 64 KiB on every rung of its ladder; and
the host wrappers refuse bad arguments before any launch (made-up addresses, nothing dereferenced:
every call below is one the library must turn down)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from trlx_t5_amd import _lib
from golden_util import T
from oracle import ppo_oracle as orc
import ppo_token_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trlx_t5_amd.h")
TOKEN_ROWS = os.path.join(ROOT, "trlx-t5_amd", "csrc", "token_rows.hip")
OK, ERR_SHAPE, ERR_DTYPE, ERR_ARG = 0, 1, 3, 5
BASE, S = 0x7000_0000_0000, 1 << 24  # made-up device addresses
LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "trlx-t5_amd", "csrc"), "-j8"])
    return _lib.load()


def close32(got64, want32, msg=""):
    torch.testing.assert_close(got64.float(), want32.float(), **C.RT32, msg=lambda m: f"{msg}: {m}")


# ------------------------------------------------------------------ the restatements against the fixtures
@pytest.mark.parametrize("mode", ["none", "running", "ref"])
def test_kl_reward64_reproduces_the_fixture(golden, mode):
    z = golden("kl_reward")
    lp = orc.logprobs_from_logits(T(z["f32/logits"]), T(z["f32/labels"]))
    rlp = orc.logprobs_from_logits(T(z["f32/ref_logits"]), T(z["f32/labels"]))
    got = C.kl_reward64(lp, rlp, float(z["f32/beta"]), T(z[f"f32/{mode}/scores_out"]))
    close32(got, T(z[f"f32/{mode}/rewards"]))
    # lengths = T everywhere is the same thing
    full = torch.full((lp.shape[0],), lp.shape[1], dtype=torch.int64)
    assert torch.equal(got, C.kl_reward64(lp, rlp, float(z["f32/beta"]), T(z[f"f32/{mode}/scores_out"]), full))


def test_gae64_reproduces_the_fixture(golden):
    z = golden("gae")
    keys = sorted({k.split("/")[0] for k in z.files if "float32" in k})
    assert len(keys) == 12
    for k in keys:
        v, r = T(z[f"{k}/values"]), T(z[f"{k}/rewards"])
        adv, ret, rec = C.gae64(v, r, v.shape[1], float(z[f"{k}/gamma"]), float(z[f"{k}/lam"]))
        assert rec[2] == v.numel() == rec[3]
        if k.endswith("_w1"):
            adv = C.whiten64(adv)
        close32(adv, T(z[f"{k}/adv"]), k)
        close32(ret, T(z[f"{k}/ret"]), k)


@pytest.mark.parametrize("name", ["f32", "f32_big"])
def test_whiten64_reproduces_the_fixture(golden, name):
    z = golden("whiten")
    xs = T(z[f"{name}/xs"])
    close32(C.whiten64(xs), T(z[f"{name}/nodist"]))
    close32(C.whiten64(xs, shift_mean=False), T(z[f"{name}/nodist_noshift"]))
    # biased against the oracle's one-rank global_statistics; n = 1: NaN like torch.var_mean
    close32(C.whiten64(xs, unbiased=False), C.whiten32(xs, unbiased=False))
    assert torch.isnan(C.whiten64(torch.tensor([3.0]))).all() and torch.isnan(C.whiten32(torch.tensor([3.0]))).all()
    m = C.moments64(xs)
    assert m[2] == xs.numel() and m[3] == 0 and m[0] == pytest.approx(float(xs.double().sum()), rel=1e-12)


@pytest.mark.parametrize("case", ["random", "masked", "ties", "wide_ratio", "vf_coef"])
def test_ppo_loss64_reproduces_the_fixture(golden, case):
    z = golden("ppo_loss")
    g = {n: T(z[f"{case}/{n}"]) for n in ("lp", "olp", "v", "ov", "adv", "ret", "mask")}
    got = C.ppo_loss64(g["lp"], g["v"], g["olp"], g["ov"], g["adv"], g["ret"], g["mask"],
                       vf_coef=float(z[f"{case}/vf_coef"]))
    want_stats = torch.tensor([float(z[f"{case}/stats/{k}"]) for k in C.STATS_KEYS])
    close32(got["dlp"], T(z[f"{case}/grad_lp"]), "dlp")
    if case == "ties":
        # rows 0-1 put v on ov +- 0.2 as fp32 rounds it: no tie in float64, so the value side (dv,
        # value loss, clipfrac) is compared on the rows whose ties are exact in both precisions
        close32(got["dv"][2:], T(z[f"{case}/grad_v"])[2:], "dv")
        keep = [i for i, k in enumerate(C.STATS_KEYS) if k not in ("values/clipfrac",)]
        close32(got["stats"][keep], want_stats[keep], "stats")
    else:
        close32(got["dv"], T(z[f"{case}/grad_v"]), "dv")
        close32(got["stats"], want_stats, "stats")
        close32(got["stats"][0], T(z[f"{case}/loss"]), "loss")


def test_loss64_with_adv_stats_is_whiten_then_loss():
    d = C.loss_inputs(45, 1, seed=3, mask="random")
    m = C.moments64(d["adv"])
    for unbiased in (True, False):
        a = C.ppo_loss64(d["lp"], d["v"], d["olp"], d["ov"], d["adv"], d["ret"], d["mask"], adv_stats=m[:3],
                         unbiased=unbiased)
        b = C.ppo_loss64(d["lp"], d["v"], d["olp"], d["ov"], C.whiten64(d["adv"], unbiased), d["ret"], d["mask"])
        for k in a:
            torch.testing.assert_close(a[k], b[k], rtol=1e-12, atol=1e-14)
        w = C.ppo_loss32(d["lp"], d["v"], d["olp"], d["ov"], d["adv"], d["ret"], d["mask"], adv_stats=m[:3],
                         unbiased=unbiased)
        assert C.figures(C.compare(w, a))["dlp"] < 1e-6


def test_lengths_restatements_agree_with_the_oracle_in_fp32():
    B, Tn = 9, 6
    lp, ref, sc = C.kl_inputs(B, Tn, seed=4)
    ln = C.edge_lengths(B, Tn, seed=5)
    assert {0, 1, Tn} <= set(ln.tolist())
    r64, r32 = C.kl_reward64(lp, ref, 0.05, sc, ln), C.kl_reward32(lp, ref, 0.05, sc, ln)
    close32(r64, r32)
    assert bool((r32[ln == 0] == 0).all()) and bool((r64[C.pad_mask(ln, Tn)] == 0).all())
    v, r = C.gae_inputs(B, Tn + 2, seed=6)
    a64, t64, rec = C.gae64(v, r, Tn, 0.99, 0.99, ln, mask=torch.ones(B, Tn, dtype=torch.int64))
    a32, t32 = C.gae32(v, r, Tn, 0.99, 0.99, ln)
    close32(a64, a32)
    close32(t64, t32)
    assert bool((a64[ln == 0] == 0).all()) and rec[2] == B * Tn == rec[3]


# ------------------------------------------------------------------ the acceptance rule
def test_the_rule_rejects_a_wrong_result_and_accepts_the_oracle():
    d = C.loss_inputs(513, 1, seed=8, mask="random")
    args = [d[k] for k in ("lp", "v", "olp", "ov", "adv", "ret", "mask")]
    want, ref = C.ppo_loss64(*args), C.ppo_loss32(*args)
    e_ref = C.compare(ref, want)
    assert C.accepted(e_ref, e_ref) and all(0 < v < 1e-5 for v in C.figures(e_ref).values())
    for k in ("stats", "dlp", "dv"):
        bad = {n: t.clone() for n, t in ref.items()}
        bad[k].view(-1)[int(bad[k].abs().argmax())] *= 1 + 2e-5
        assert not C.accepted(C.compare(bad, want), e_ref), k
    nan = {n: t.clone() for n, t in ref.items()}
    nan["dv"].view(-1)[3] = float("nan")
    assert C.compare(nan, want)["dv"] == float("inf")
    # an exact oracle leaves the kernel one fp32 ulp of the largest magnitude
    w = {"x": torch.tensor([1.5, -3.0], dtype=torch.float64)}
    zero = C.compare({"x": w["x"].clone()}, w)
    assert zero["x"] == 0.0
    assert C.accepted(C.compare({"x": w["x"] + torch.tensor([0.0, 2.0 ** -22])}, w), zero)
    assert not C.accepted(C.compare({"x": w["x"] + torch.tensor([0.0, 2.0 ** -21])}, w), zero)
    # bf16: one bf16 ulp around the once-rounded float64 value
    x = torch.tensor([1.0 + 2.0 ** -9, -0.3], dtype=torch.float64)
    r = x.to(torch.bfloat16)
    assert C.bf16_close(r, x) and C.bf16_close((r.float() * (1 + 2.0 ** -7)).to(torch.bfloat16), x)
    assert not C.bf16_close((r.float() * (1 + 2.0 ** -6)).to(torch.bfloat16), x)


# ------------------------------------------------------------------ the tie generator
def test_tie_generator_plants_what_it_claims():
    n = 1061
    d, planted = C.tie_inputs(n, seed=9)
    got = C.count_ties(d)
    plain = C.count_ties(C.loss_inputs(n, 1, seed=9))
    assert all(v == 0 for v in plain.values()), plain  # nothing of the kind without planting
    names = ["v_lo", "v_hi", "ratio_lo", "ratio_hi", "adv0", "vl_tie_outside"]
    assert [got[k] for k in names] == [len(planted[i]) for i in range(6)], (got, {k: len(v) for k, v in planted.items()})
    assert len(planted[0]) == len(planted[1]) == len(planted[4]) == (n + 7) // 8 or len(planted[4]) == n // 8
    assert min(len(planted[i]) for i in range(6)) >= 20, {k: len(v) for k, v in planted.items()}
    # the reference's rules at those positions: torch.maximum halves the gradient on a tie and
    # clamp passes it on an inclusive bound (fp32 oracle autograd)
    ref = C.ppo_loss32(d["lp"], d["v"], d["olp"], d["ov"], d["adv"], d["ret"], d["mask"])
    u = 1.0 / n
    for i in planted[0] + planted[1]:  # v on the bound: vclip == v, both branches carry e·u/… -> full gradient
        e = float(d["v"][i, 0] - d["ret"][i, 0])
        assert float(ref["dv"][i, 0]) == pytest.approx(u * e, rel=1e-5, abs=1e-9)
    for i in planted[5]:  # tie with v outside: only the unclipped branch's half
        e = float(d["v"][i, 0] - d["ret"][i, 0])
        assert float(ref["dv"][i, 0]) == pytest.approx(0.5 * u * e, rel=1e-5, abs=1e-9)
    for i in planted[2] + planted[3]:  # ratio on the bound: pg1 == pg2, clamp passes: the full -A·ratio/n
        ratio = float(torch.exp(d["lp"][i, 0] - d["olp"][i, 0]))
        assert float(ref["dlp"][i, 0]) == pytest.approx(-float(d["adv"][i, 0]) * ratio * u, rel=1e-5, abs=1e-9)
    assert all(float(ref["dlp"][i, 0]) == 0.0 for i in planted[4])


# ------------------------------------------------------------------ gamma * lam
def test_gamma_lam_cross_the_abi_as_doubles():
    """fl32(gamma * lam) needs the double product: rounding the factors to fp32 first moves it by an
    ulp for five of the pairs (the GPU test's bit-equality of the advantages is what observes the
    value the library forms)."""
    f32 = np.float32
    off = [(g, l) for g, l in C.GL_PAIRS if f32(float(f32(g)) * float(f32(l))) != f32(g * l)]
    assert off == C.GL_PAIRS[2:]
    assert float(f32(0.99 * 0.99)) == 0.9800999760627747
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.search(r"float\s+(gamma|lam)\b", txt) and "double gamma, lam;" in txt  # (ILQL's own gamma aside)
    assert len(re.findall(r"double gamma, double lam|double gamma,\s+double lam", txt)) == 5
    # every declaration that takes them: the binding has c_double at those two positions and
    # c_double nowhere a float or pointer stands (a c_float there would hand the callee garbage)
    decls = re.findall(r"^int (trlx_\w+)\(([^;]*?double gamma,\s+double lam[^;]*?)\);", txt, flags=re.M | re.S)
    assert sorted(n for n, _ in decls) == ["trlx_gae_scan", "trlx_ppo_experience_fused", "trlx_ppo_rollout_gae",
                                           "trlx_ppo_rollout_gae_ctl", "trlx_ppo_rollout_gae_split"]
    for name, args in decls:
        params = [" ".join(a.split()) for a in args.split(",")]
        sig = _lib.SIGNATURES[name][1]
        assert len(sig) == len(params), name
        for a, ct in zip(params, sig):
            assert (ct is _lib._c_d) == a.startswith("double "), (name, a)
            assert (ct is _lib._c_f) == a.startswith("float "), (name, a)
    assert dict(_lib.GaeSplitArgs._fields_)["gamma"] is _lib._c_d and dict(_lib.GaeSplitArgs._fields_)["lam"] is _lib._c_d


# ------------------------------------------------------------------ GAE launch geometry
def static_lds_bytes():
    m = re.search(r"constexpr int kGaeStaticLdsBytes = (\d+);", open(TOKEN_ROWS).read())
    assert m
    return int(m.group(1))


def lds_total(rpb, teff):
    return 2 * rpb * ((teff + 1) | 1) * 4 + static_lds_bytes()


def largest_admitted():
    t = 1
    while lds_total(1, t + 1) <= LDS_LIMIT:
        t += 1
    return t


def rows_per_block(lib, teff):
    """rpb from the block counts of B = 1..17: blocks = ceil(B / rpb)."""
    nb = [lib.trlx_gae_num_blocks(B, teff) for B in range(1, 18)]
    rpb = max(B for B, k in zip(range(1, 18), nb) if k == 1)
    assert nb == [-(-B // rpb) for B in range(1, 18)], (teff, nb)
    return rpb


def test_gae_geometry_fits_64k_with_the_static_part(lib):
    static = static_lds_bytes()
    assert static >= 144  # the compiler's report for k_gae (make resources RES_SRC=token_rows.hip)
    last = largest_admitted()
    assert last == 8172
    seen = {}
    for teff in (1, 256, 508, 509, 510, 511, 544, 545, 2728, 2729, 4094, 4095, last):
        rpb = rows_per_block(lib, teff)
        assert lds_total(rpb, teff) <= LDS_LIMIT, (teff, rpb)
        assert rpb == 16 or lds_total(rpb + 1, teff) > LDS_LIMIT, (teff, rpb)
        seen[teff] = rpb
    assert seen[508] == 16 and seen[509] == seen[510] == 15 and seen[4095] == 1 and seen[last] == 1
    assert set(seen.values()) == {16, 15, 14, 2, 1}  # the rungs these lengths stand on
    # the first refused length: not even one row fits, and the scan is turned down before a launch
    assert lds_total(1, last + 1) > LDS_LIMIT
    rc, msg = gae_call(lib, B=2, T=last + 1, Teff=last + 1)
    assert rc == ERR_SHAPE and "too long" in msg
    # every length the old dynamic-only check let through over the limit now fits
    for teff in range(1, last + 1):
        old_rpb = max(1, min(16, 8192 // ((teff + 1) | 1)))
        if lds_total(old_rpb, teff) > LDS_LIMIT:
            assert lds_total(rows_per_block(lib, teff), teff) <= LDS_LIMIT, teff


# ------------------------------------------------------------------ refusals, nothing launched
def gae_call(lib, **over):
    a = dict(values=BASE, rewards=BASE + S, dtype=_lib.F32, B=4, T=8, Teff=8, gamma=0.99, lam=0.95, lp=None,
             ref_lp=None, neg_beta=0.0, scores=None, lengths=None, mask=None, adv=BASE + 2 * S, ret=BASE + 3 * S,
             ret_dtype=_lib.F32, rew_out=None, rew_dtype=_lib.F32, partials=BASE + 4 * S, stats=BASE + 5 * S,
             ticket=BASE + 6 * S, stream=None)
    assert over, "a call with nothing wrong would launch"
    a.update(over)
    rc = lib.trlx_gae_scan(*a.values())
    return rc, lib.trlx_last_error().decode()


@pytest.mark.parametrize("over, code, word", [
    (dict(T=9000, Teff=8173), ERR_SHAPE, "too long"),
    (dict(T=9000, Teff=8190), ERR_SHAPE, "too long"),
    (dict(T=1 << 20, Teff=1 << 20), ERR_SHAPE, "too long"),
    (dict(T=8, Teff=9), ERR_SHAPE, "bad shape"),
    (dict(Teff=0), ERR_SHAPE, "bad shape"),
    (dict(B=0), ERR_SHAPE, "bad shape"),
    (dict(B=1 << 20, T=1 << 11, Teff=1), ERR_SHAPE, "bad shape"),
    (dict(lp=BASE + 7 * S, ref_lp=BASE + 8 * S, Teff=4), ERR_SHAPE, "fused KL reward"),
    (dict(ticket=None), ERR_ARG, "ticket"),
    (dict(values=None), ERR_ARG, "NULL"),
    (dict(adv=None), ERR_ARG, "NULL"),
    (dict(ret=None), ERR_ARG, "NULL"),
    (dict(partials=None), ERR_ARG, "NULL"),
    (dict(rewards=None), ERR_ARG, "need rewards"),
    (dict(rewards=None, lp=BASE + 7 * S), ERR_ARG, "need rewards"),
])
def test_gae_scan_refusals(lib, over, code, word):
    rc, msg = gae_call(lib, **over)
    assert rc == code and word in msg, (rc, msg)


def loss_call(lib, **over):
    a = dict(n=100, lp=BASE, lp_dtype=_lib.F32, v=BASE + S, v_dtype=_lib.F32, olp=BASE + 2 * S, olp_dtype=_lib.F32,
             ov=BASE + 3 * S, ov_dtype=_lib.F32, adv=BASE + 4 * S, a_dtype=_lib.F32, adv_stats=None, unbiased=1,
             ret=BASE + 5 * S, r_dtype=_lib.F32, mask=None, msum=None, msum_host=100.0, c=0.2, cv=0.2, vf_coef=1.0,
             dlp=BASE + 6 * S, dv=BASE + 7 * S, g_dtype=_lib.F32, partials=BASE + 8 * S, loss=BASE + 9 * S,
             stats=BASE + 10 * S, ticket=BASE + 11 * S, stream=None)
    assert over, "a call with nothing wrong would launch"
    a.update(over)
    rc = lib.trlx_ppo_loss_elem(*a.values())
    return rc, lib.trlx_last_error().decode()


@pytest.mark.parametrize("over, code, word", [
    (dict(n=0), ERR_SHAPE, "empty"),
    (dict(n=-5), ERR_SHAPE, "empty"),
    (dict(loss=None), ERR_ARG, "needs loss and stats"),
    (dict(stats=None), ERR_ARG, "needs loss and stats"),
    (dict(msum_host=0.0), ERR_ARG, "mask sum"),
    (dict(msum_host=-1.0), ERR_ARG, "mask sum"),
    (dict(lp=None), ERR_ARG, "NULL"),
    (dict(partials=None), ERR_ARG, "NULL"),
])
def test_ppo_loss_elem_refusals(lib, over, code, word):
    rc, msg = loss_call(lib, **over)
    assert rc == code and word in msg, (rc, msg)


def test_other_token_entries_refuse_before_launching(lib):
    for dt in (3, -1, 7):
        assert lib.trlx_moments_partial(BASE, dt, 10, BASE + S, None) == ERR_DTYPE
        assert f"dtype {dt}" in lib.trlx_last_error().decode()
    assert lib.trlx_moments_partial(None, _lib.F32, 10, BASE + S, None) == ERR_ARG
    assert lib.trlx_moments_partial(BASE, _lib.F32, -1, BASE + S, None) == ERR_SHAPE
    assert lib.trlx_moments_finalize(BASE, 0, BASE + S, None) == ERR_ARG
    assert lib.trlx_ppo_loss_finalize(BASE, 0, 10, None, 10.0, 1.0, BASE + S, BASE + 2 * S, None) == ERR_ARG
    assert lib.trlx_ppo_loss_finalize(BASE, 1, 10, None, 10.0, 1.0, None, BASE + 2 * S, None) == ERR_ARG
    assert lib.trlx_kl_penalty_rewards(BASE, None, _lib.F32, 2, 2, 0.1, None, None, BASE + S, _lib.F32, None) == ERR_ARG
    assert lib.trlx_kl_penalty_rewards(BASE, BASE + S, _lib.F32, -1, 2, 0.1, None, None, BASE + 2 * S, _lib.F32,
                                       None) == ERR_SHAPE
    # nothing to do is not an error and launches nothing
    assert lib.trlx_kl_penalty_rewards(BASE, BASE + S, _lib.F32, 0, 5, 0.1, None, None, BASE + 2 * S, _lib.F32, None) == OK
    assert lib.trlx_whiten_apply(BASE, _lib.F32, 0, BASE + S, 1, 1, BASE + 2 * S, _lib.F32, None) == OK
    assert lib.trlx_scale_by(BASE, BASE, _lib.F32, 0, BASE + S, None) == OK
    assert lib.trlx_scale_by(BASE, BASE, _lib.F32, 5, None, None) == ERR_ARG
