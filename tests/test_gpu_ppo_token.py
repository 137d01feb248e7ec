"""The [B, T] PPO token kernels on the GPU: token_rows.hip (k_kl_rewards, k_gae, k_moments_partial,
k_moments_finalize, k_whiten_apply) and ppo_loss.hip (k_ppo_loss_elem, k_ppo_loss_finalize,
k_scale_by), through the drop-in API and, for what it does not reach, through the C ABI.

Shapes are the smallest that reach each launch geometry: one element, one below / at / above a
block (256 threads elementwise, 512 tokens of the loss, 4096 elements of the moments), more
records than the reducing block has threads (257 / 258 blocks), one element-lap past the
elementwise grid caps (4096 x 256, 8192 x 256 for scale_by), and every rung change of the GAE's
rows-per-block ladder up to the longest admitted response.

Where the kernel performs the reference's fp32 operations in the reference's order (KL reward, raw
GAE) the result must be bit-equal to the fp32 oracle.  Elsewhere accuracy is measured, not
toleranced: ppo_token_checks.compare / accepted (kernel error against float64 at most twice the
fp32 oracle's).  bf16 outputs: within one bf16 ulp of the float64 result rounded once.  Buffers
handed to the C ABI directly carry 24 sentinel elements on both sides, which must survive.
TRLX_PPO_TOKEN_PARITY_OUT=<file>: the measured figures are written there
(profiles/ppo_token_parity.json is such a run)."""
import json
import math
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import ppo_token_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
SENTINEL, PAD = 12288.0, 24  # exact in bf16 too
_FIGURES = {}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    yield
    path = os.environ.get("TRLX_PPO_TOKEN_PARITY_OUT")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "e_kernel <= 2 * e_ref32 per output (one fp32 ulp of the output's largest magnitude "
                               "where e_ref32 == 0); e_* = max error against the float64 restatement "
                               "(tests/ppo_token_checks.py: max |x - x64| over each output buffer; stats = the 13 "
                               "loss stats, element 0 the loss), e_ref32 = oracle/ppo_oracle.py in fp32 on the CPU",
                       "cases": [dict(case=k, **_FIGURES[k]) for k in sorted(_FIGURES)]}, f, indent=1)


def cuda(t):
    return None if t is None else t.to(DEV)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def check_rule(case, got, ref32, want64):
    e_k, e_r = C.compare(got, want64), C.compare(ref32, want64)
    print(case, "e_kernel", C.figures(e_k), "e_ref32", C.figures(e_r))
    _FIGURES[case] = {"e_kernel": C.figures(e_k), "e_ref32": C.figures(e_r)}
    assert all(math.isfinite(v) for v in C.figures(e_k).values()), (case, e_k)
    assert C.accepted(e_k, e_r), (case, C.figures(e_k), C.figures(e_r))


class Guarded:
    """A sentinel-filled device buffer with PAD elements of slack on both sides of the result."""

    def __init__(self, n, dtype):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + self.n]

    def ptr(self):
        return self.view.data_ptr()

    def result(self, shape=None):
        torch.cuda.synchronize()
        assert bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all()), \
            "written outside the result"
        out = self.view.clone()
        return out if shape is None else out.view(shape)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2
                               else torch.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ================================================================== KL reward
def run_kl(lp, ref, beta, scores, lengths, out_dtype):
    """trlx_kl_penalty_rewards into a guarded buffer (any in / out dtype pair)."""
    lp, ref, sc, ln = cuda(lp).contiguous(), cuda(ref).contiguous(), cuda(scores), cuda(lengths)
    B, T = lp.shape
    out = Guarded(B * T, out_dtype)
    _lib.call("trlx_kl_penalty_rewards", lp.data_ptr(), ref.data_ptr(), _lib.dtype_code(lp), B, T, float(beta),
              _lib.ptr(sc), _lib.ptr(ln), out.ptr(), _lib.dtype_code(out.view), stream())
    return out.result((B, T))


KL_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (37, 7), (3, 1), (1048581, 1), (149798, 7)]


@pytest.mark.parametrize("with_scores, with_lengths", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B, T", KL_SHAPES)
def test_kl_reward_fp32_is_bit_equal_to_the_oracle(B, T, with_scores, with_lengths):
    """Each output is -beta * (lp - ref_lp) [+ score]: the same one to three IEEE operations in the
    oracle's order.  (149798 x 7 and 1048581 x 1 are past the 4096 x 256 grid: the second lap.)"""
    lp, ref, sc = C.kl_inputs(B, T, seed=B + T)
    ln = C.edge_lengths(B, T, seed=B) if with_lengths else None
    sc = sc if with_scores else None
    got = P.kl_penalty_rewards(cuda(lp), cuda(ref), 0.05, cuda(sc), cuda(ln))
    want = C.kl_reward32(lp, ref, 0.05, sc, ln)
    assert same_bits(got, want)
    assert same_bits(run_kl(lp, ref, 0.05, sc, ln, F32), want)


@pytest.mark.parametrize("B, T", [(257, 1), (37, 7), (149798, 7)])
def test_kl_reward_other_dtypes(B, T):
    lp, ref, sc = C.kl_inputs(B, T, seed=B + T, dtype=BF16)
    ln = C.edge_lengths(B, T, seed=B)
    want64 = C.kl_reward64(lp, ref, 0.05, sc, ln)
    got = P.kl_penalty_rewards(cuda(lp), cuda(ref), 0.05, cuda(sc), cuda(ln))  # bf16 -> bf16
    assert got.dtype == BF16 and C.bf16_close(got, want64)
    assert same_bits(run_kl(lp, ref, 0.05, sc, ln, BF16), got.cpu())
    # bf16 -> fp32: the oracle's fp32 operations on the exact bf16 values
    assert same_bits(run_kl(lp, ref, 0.05, sc, ln, F32), C.kl_reward32(lp, ref, 0.05, sc, ln))
    # fp32 -> bf16
    lp32, ref32, _ = C.kl_inputs(B, T, seed=B + T)
    assert C.bf16_close(run_kl(lp32, ref32, 0.05, sc, ln, BF16), C.kl_reward64(lp32, ref32, 0.05, sc, ln))


# ================================================================== GAE
def run_gae(v, r, Teff, gamma, lam, lengths=None, mask=None, lp=None, ref=None, beta=0.0, scores=None,
            rew_dtype=None, with_stats=True, ticket=None):
    """trlx_gae_scan with every output guarded.  rew_dtype None: rew_out NULL."""
    v = cuda(v).contiguous()
    r, lp, ref = (None if t is None else cuda(t).contiguous() for t in (r, lp, ref))
    B, T = v.shape
    nblk = _lib.query("trlx_gae_num_blocks", B, Teff)
    adv, ret = Guarded(B * Teff, F32), Guarded(B * Teff, v.dtype)
    part, st = Guarded(nblk * 4, torch.float64), Guarded(4, torch.float64)
    rew = None if rew_dtype is None else Guarded(B * T, rew_dtype)
    tk = ticket if ticket is not None else torch.zeros(1, dtype=torch.int32, device=DEV)
    ln, mk, sc = cuda(lengths), cuda(mask), cuda(scores)
    _lib.call("trlx_gae_scan", v.data_ptr(), _lib.ptr(r), _lib.dtype_code(v), B, T, Teff, float(gamma), float(lam),
              _lib.ptr(lp), _lib.ptr(ref), -float(beta), _lib.ptr(sc), _lib.ptr(ln), _lib.ptr(mk), adv.ptr(), ret.ptr(),
              _lib.dtype_code(v), None if rew is None else rew.ptr(), _lib.F32 if rew is None else _lib.dtype_code(rew.view),
              part.ptr(), st.ptr() if with_stats else None, tk.data_ptr() if with_stats else None, stream())
    return dict(adv=adv.result((B, Teff)), ret=ret.result((B, Teff)), rew=None if rew is None else rew.result((B, T)),
                partials=part.result(), stats=st.result(), ticket=tk, nblk=nblk)


def record_of(adv32, n_mask=None):
    """The moment record of the fp32 advantages, summed exactly."""
    a = adv32.double().reshape(-1)
    n = float(a.numel())
    return [math.fsum(a.tolist()), math.fsum((a * a).tolist()), n, n if n_mask is None else float(n_mask)]


def check_record(st, adv32, n_mask=None):
    want = record_of(adv32, n_mask)
    got = st.cpu().tolist()
    assert got[2] == want[2] and got[3] == want[3], (got, want)
    assert got[0] == pytest.approx(want[0], rel=1e-12) and got[1] == pytest.approx(want[1], rel=1e-12), (got, want)


def gae_reference(B, Teff, gl, T=None, lengths=False, dtype=F32):
    def make():
        v, r = C.gae_inputs(B, T or Teff, seed=B * 10007 + Teff, dtype=dtype)
        ln = C.edge_lengths(B, Teff, seed=B + Teff) if lengths else None
        a32, r32 = C.gae32(v, r, Teff, gl[0], gl[1], ln)
        return v, r, ln, a32, r32
    return cached(("gae", B, Teff, gl, T, lengths, dtype), make)


GAE_SHAPES = [(17, 1), (17, 2), (17, 255), (17, 256), (17, 257), (31, 510), (31, 511), (29, 545), (5, 2729),
              (3, 4094), (3, 4095), (2, 8172), (4113, 1)]
GLS = [(0.99, 0.99), (1.0, 0.95)]


@pytest.mark.parametrize("gl", GLS)
@pytest.mark.parametrize("B, Teff", GAE_SHAPES)
def test_gae_raw_fp32_is_bit_equal_to_the_oracle_loop(B, Teff, gl):
    """Same operations, same order, no fma, and gamma*lam rounded to fp32 once: the advantages and
    returns are the oracle loop's bits on every rung of the rows-per-block ladder (16 rows up to
    Teff 508, 15 at 509-543, 14 from 544, 2 at 2728, 1 from 2729 to the longest admitted 8172; 4113
    rows of one token make 258 records for the 256 reducing threads)."""
    v, r, _, a32, r32 = gae_reference(B, Teff, gl)
    cfg = P.PPOConfig(gamma=gl[0], lam=gl[1])
    adv, ret, st = cfg.gae_raw(cuda(v), cuda(r), Teff)
    assert same_bits(adv, a32) and same_bits(ret, r32)
    check_record(st, a32)


@pytest.mark.parametrize("gl", C.GL_PAIRS)
def test_gae_gamma_lam_product_is_rounded_once(gl):
    v, r, _, a32, r32 = gae_reference(17, 257, gl)
    adv, ret, _ = P.PPOConfig(gamma=gl[0], lam=gl[1]).gae_raw(cuda(v), cuda(r), 257)
    assert same_bits(adv, a32) and same_bits(ret, r32)


@pytest.mark.parametrize("gl", GLS)
def test_gae_response_shorter_than_the_row(gl):
    v, r, _, a32, r32 = gae_reference(17, 257, gl, T=262)
    adv, ret, st = P.PPOConfig(gamma=gl[0], lam=gl[1]).gae_raw(cuda(v), cuda(r), 257)
    assert same_bits(adv, a32) and same_bits(ret, r32)
    check_record(st, a32)
    out = run_gae(v, r, 257, *gl)
    assert same_bits(out["adv"], a32) and same_bits(out["ret"], r32)


@pytest.mark.parametrize("gl", GLS)
@pytest.mark.parametrize("B, Teff", [(17, 257), (31, 511), (5, 2729)])
def test_gae_bf16_values_and_returns(B, Teff, gl):
    """fp32 arithmetic on the exact bf16 values, the returns rounded to bf16 once at the store.
    The one-bf16-ulp rule against float64 is asked on inputs with rewards >= 0.05 and values >= 0:
    there returns_t = r_t + gamma (1 - lam) V_{t+1} + gamma lam returns_{t+1} is a sum of positive
    terms >= 0.05, far above the fp32 error of the scan.  On N(0, 1) values A + V cancels to
    returns smaller than that error (one bf16 ulp of 1e-6 is 4e-9), where no fp32 evaluation can
    meet the rule; there the returns must be the fp32 oracle's returns rounded to bf16, bit for bit."""
    cfg = P.PPOConfig(gamma=gl[0], lam=gl[1])
    v, r, _, a32, r32 = gae_reference(B, Teff, gl, dtype=BF16)
    adv, ret, st = cfg.gae_raw(cuda(v), cuda(r), Teff)
    assert adv.dtype == F32 and ret.dtype == BF16
    assert same_bits(adv, a32) and same_bits(ret, r32.to(BF16))
    check_record(st, a32)
    g = C.gen(B + Teff)
    vp = torch.rand(B, Teff, generator=g).to(BF16)
    rp = (0.05 + 0.2 * torch.rand(B, Teff, generator=g)).to(BF16)
    assert float(rp.min()) >= 0.05
    adv, ret, _ = cfg.gae_raw(cuda(vp), cuda(rp), Teff)
    a32, r32 = C.gae32(vp, rp, Teff, *gl)
    assert same_bits(adv, a32) and same_bits(ret, r32.to(BF16))
    assert C.bf16_close(ret, C.gae64(vp, rp, Teff, *gl)[1])


@pytest.mark.parametrize("gl", GLS)
def test_gae_lengths_and_mask(gl):
    B, Teff = 31, 511
    v, r, ln, a32, r32 = gae_reference(B, Teff, gl, lengths=True)
    assert {0, 1, Teff} <= set(ln.tolist())
    mask = torch.randint(0, 2, (B, Teff), generator=C.gen(77))
    adv, ret, st = P.PPOConfig(gamma=gl[0], lam=gl[1]).gae_raw(cuda(v), cuda(r), Teff, lengths=cuda(ln), mask=cuda(mask))
    assert same_bits(adv, a32) and same_bits(ret, r32)
    assert bool((adv.cpu()[ln == 0] == 0).all())
    check_record(st, a32, n_mask=int(mask.sum()))


@pytest.mark.parametrize("rew_dtype", [F32, BF16, None])
@pytest.mark.parametrize("gl", GLS)
def test_gae_fused_kl_reward_equals_the_two_launches(gl, rew_dtype):
    B, T = 31, 511
    lp, ref, sc = C.kl_inputs(B, T, seed=5)
    v, _ = C.gae_inputs(B, T, seed=6)
    ln = C.edge_lengths(B, T, seed=7)
    rewards = P.kl_penalty_rewards(cuda(lp), cuda(ref), 0.05, cuda(sc), cuda(ln))
    adv, ret, st = P.PPOConfig(gamma=gl[0], lam=gl[1]).gae_raw(cuda(v), rewards, T, lengths=cuda(ln))
    out = run_gae(v, None, T, *gl, lengths=ln, lp=lp, ref=ref, beta=0.05, scores=sc, rew_dtype=rew_dtype)
    assert same_bits(out["adv"], adv) and same_bits(out["ret"], ret) and same_bits(out["stats"], st)
    if rew_dtype is not None:
        assert same_bits(out["rew"], rewards.to(rew_dtype))
    # and against the oracle: rewards, then the loop
    a32, r32 = C.gae32(v, C.kl_reward32(lp, ref, 0.05, sc, ln), T, *gl, ln)
    assert same_bits(adv, a32) and same_bits(ret, r32)


@pytest.mark.parametrize("B, Teff", [(31, 511), (4113, 1)])
def test_gae_without_stats_writes_exactly_its_records_and_the_ticket_rearms(B, Teff):
    gl = GLS[0]
    v, r, _, a32, _ = gae_reference(B, Teff, gl)
    first = run_gae(v, r, Teff, *gl)
    assert int(first["ticket"].cpu()) == 0  # re-armed by the last block
    again = run_gae(v, r, Teff, *gl, ticket=first["ticket"])
    for k in ("adv", "ret", "stats", "partials"):
        assert same_bits(first[k], again[k]), k
    assert int(again["ticket"].cpu()) == 0
    plain = run_gae(v, r, Teff, *gl, with_stats=False)
    assert plain["nblk"] == _lib.query("trlx_gae_num_blocks", B, Teff) and plain["partials"].numel() == 4 * plain["nblk"]
    assert not bool((plain["partials"] == SENTINEL).any())  # every record written (Guarded: and nothing else)
    assert bool((plain["stats"] == SENTINEL).all())         # stats untouched
    assert same_bits(plain["adv"], first["adv"]) and same_bits(plain["partials"], first["partials"])
    tot = plain["partials"].view(-1, 4).cpu()
    want = first["stats"].cpu().tolist()
    for k in range(4):
        assert math.fsum(tot[:, k].tolist()) == pytest.approx(want[k], rel=1e-12)
    check_record(first["stats"], a32)


# ================================================================== moments
def run_moments(x):
    x = cuda(x).contiguous()
    n = x.numel()
    nblk = _lib.query("trlx_moments_num_blocks", n)
    part, st = Guarded(nblk * 4, torch.float64), Guarded(4, torch.float64)
    _lib.call("trlx_moments_partial", _lib.ptr(x) or None, _lib.dtype_code(x), n, part.ptr(), stream())
    _lib.call("trlx_moments_finalize", part.ptr(), nblk, st.ptr(), stream())
    return st.result().cpu().tolist(), part.result()


MOM_N = [0, 1, 4095, 4096, 4097, 4096 * 257 + 5]


def moments_input(n, dtype):
    g = C.gen(n + 1)
    if dtype == torch.int64:
        return torch.randint(-3, 5, (n,), generator=g)
    return (torch.randn(n, generator=g) * 3 + 0.5).to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF16, torch.int64])
@pytest.mark.parametrize("n", MOM_N)
def test_moments(n, dtype):
    """One block takes 4096 elements: 4097 is two blocks, 4096·257 + 5 is 258 records for the 256
    threads of the finalize."""
    x = moments_input(n, dtype)
    want = C.moments64(x)
    got, part = run_moments(x)
    assert part.numel() == 4 * max(1, -(-n // 4096)) and not bool((part == SENTINEL).any())
    assert got[2] == n and got[3] == 0.0
    if dtype == torch.int64:
        assert got[0] == want[0] and got[1] == want[1]  # exact
    else:
        assert got[0] == pytest.approx(want[0], rel=1e-12) and got[1] == pytest.approx(want[1], rel=1e-12)
    assert P.moments(cuda(x)).cpu().tolist() == got


def test_moments_of_a_non_contiguous_input():
    x = moments_input(2 * 4097, F32).view(4097, 2)
    got = P.moments(cuda(x)[:, 1]).cpu().tolist()
    want = C.moments64(x[:, 1])
    assert got[2] == 4097 and got[3] == 0 and got[0] == pytest.approx(want[0], rel=1e-12)
    assert got[1] == pytest.approx(want[1], rel=1e-12)
    assert P.moments(cuda(x).t()).cpu().tolist()[2] == 2 * 4097


# ================================================================== whiten
WHITEN_N = [2, 4097, 1048576 + 3]


def whiten_reference(n, dtype, shift):
    def make():
        x = (torch.randn(n, generator=C.gen(n)) * 2 + 0.75).to(dtype)
        return x, C.whiten32(x, True, shift), C.whiten64(x, True, shift)
    return cached(("whiten", n, dtype, shift), make)


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("n", WHITEN_N)
def test_whiten_fp32(n, shift):
    x, w32, w64 = whiten_reference(n, F32, shift)
    got = P.whiten(cuda(x), shift_mean=shift)
    check_rule(f"whiten n={n} shift_mean={shift}", {"out": got}, {"out": w32}, {"out": w64})
    torch.testing.assert_close(got.cpu(), w32, **C.RT32)


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("n", WHITEN_N)
def test_whiten_bf16(n, shift):
    x, _, w64 = whiten_reference(n, BF16, shift)
    got = P.whiten(cuda(x), shift_mean=shift)
    assert got.dtype == BF16 and C.bf16_close(got, w64)


@pytest.mark.parametrize("unbiased", [1, 0])
def test_whiten_apply_direct_keeps_to_its_buffer(unbiased):
    """The C entry with the biased variance too (the distributed branch), one lap past the grid cap."""
    n = 1048576 + 3
    x, _, _ = whiten_reference(n, F32, True)
    xd = cuda(x)
    out = Guarded(n, F32)
    _lib.call("trlx_whiten_apply", xd.data_ptr(), _lib.F32, n, P.moments(xd).data_ptr(), unbiased, 1, out.ptr(), _lib.F32,
              stream())
    got = out.result()
    check_rule(f"whiten_apply n={n} unbiased={unbiased}", {"out": got}, {"out": C.whiten32(x, bool(unbiased))},
               {"out": C.whiten64(x, bool(unbiased))})


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_whiten_edges(dtype):
    one = P.whiten(torch.tensor([3.0], dtype=dtype, device=DEV))  # torch.var_mean of one element: NaN
    assert one.shape == (1,) and bool(torch.isnan(one).all())
    assert bool(torch.isnan(P.whiten(torch.tensor([3.0], dtype=dtype, device=DEV), shift_mean=False)).all())
    empty = P.whiten(torch.empty(0, dtype=dtype, device=DEV))
    torch.cuda.synchronize()
    assert empty.shape == (0,) and empty.dtype == dtype
    for n in (2, 4097):  # a constant: M2 rounds to <= 0 and is clamped; exact zeros, or the mean back
        const = torch.full((n,), 0.1, dtype=dtype, device=DEV)
        assert bool((P.whiten(const) == 0).all())
        assert torch.equal(P.whiten(const, shift_mean=False), const)


# ================================================================== PPO loss
OPERANDS = ("lp", "v", "olp", "ov", "adv", "ret")


def loss_reference(n, T, mask, bf16=(), seed=None, tie=False):
    def make():
        d = C.tie_inputs(n, seed or n)[0] if tie else C.loss_inputs(n, T, seed or n, mask, bf16)
        args = [d[k] for k in OPERANDS] + [d["mask"]]
        return d, C.ppo_loss32(*args), C.ppo_loss64(*args)
    return cached(("loss", n, T, mask, tuple(bf16), seed, tie), make)


def api_loss(d, scale=None):
    lp, v = cuda(d["lp"]).requires_grad_(True), cuda(d["v"]).requires_grad_(True)
    loss, stats = P.PPOConfig().loss(lp, v, cuda(d["olp"]), cuda(d["ov"]), cuda(d["adv"]), cuda(d["ret"]), cuda(d["mask"]),
                                     return_device_stats=True)
    (loss if scale is None else scale * loss).backward()
    assert same_bits(loss.detach().reshape(1), stats[:1])
    return dict(stats=stats.detach(), dlp=lp.grad, dv=v.grad)


LOSS_SHAPES = [(1, 1), (2, 1), (511, 1), (511, 7), (512, 1), (513, 1), (1061, 1), (512 * 257 + 3, 1)]


@pytest.mark.parametrize("mask", ["ones", "random", "single", None])
@pytest.mark.parametrize("n, T", LOSS_SHAPES)
def test_ppo_loss_fp32(n, T, mask):
    """One block takes 512 tokens: 513 is two blocks with the last-block hand-off, 512·257 + 3 is
    258 records.  n = 1: the two variances are NaN as torch.var's."""
    d, ref32, want64 = loss_reference(n, T, mask)
    got = api_loss(d)
    check_rule(f"loss n={n} T={T} mask={mask}", got, ref32, want64)
    if n == 1:
        assert bool(torch.isnan(got["stats"][[4, 11]]).all()) and bool(torch.isfinite(got["stats"][[0, 1, 2]]).all())
    for k in ("stats", "dlp", "dv"):
        torch.testing.assert_close(got[k].cpu().reshape(-1), ref32[k].reshape(-1), **C.RT32, equal_nan=True)
    # grad_output = 3: k_scale_by with a scale other than 1 (one fp32 multiplication per element)
    tripled = api_loss(d, scale=3.0)
    assert same_bits(tripled["dlp"], got["dlp"] * 3.0) and same_bits(tripled["dv"], got["dv"] * 3.0)


@pytest.mark.parametrize("bf16", [(k,) for k in OPERANDS] + [OPERANDS])
def test_ppo_loss_each_operand_in_bf16(bf16):
    n = 1061
    d, ref32, want64 = loss_reference(n, 1, "random", bf16)
    got = api_loss(d)
    fp32_outs = ["stats"] + [k for k, op in (("dlp", "lp"), ("dv", "v")) if op not in bf16]
    check_rule(f"loss n={n} bf16={'+'.join(bf16)}", {k: got[k] for k in fp32_outs}, {k: ref32[k] for k in fp32_outs},
               {k: want64[k] for k in fp32_outs})
    for k, op in (("dlp", "lp"), ("dv", "v")):  # a gradient comes back in its operand's dtype
        assert got[k].dtype == d[op].dtype
        if op in bf16:
            assert C.bf16_close(got[k], want64[k]), k


def test_ppo_loss_ties_and_bounds_follow_the_reference():
    """torch.maximum splits the gradient half and half on a tie, clamp passes it on its inclusive
    bounds; the planted positions are ties in fp32 only, so the comparison is with the fp32 oracle."""
    n = 1061
    d, planted = C.tie_inputs(n, seed=n)
    _, ref32, _ = loss_reference(n, 1, "ones", tie=True)
    assert min(len(v) for v in planted.values()) >= 20
    got = api_loss(d)
    for k in ("stats", "dlp", "dv"):
        torch.testing.assert_close(got[k].cpu().reshape(-1), ref32[k].reshape(-1), **C.RT32)
    idx = torch.tensor(sorted(i for v in planted.values() for i in v))
    for k in ("dlp", "dv"):  # relative at the planted positions: half a gradient would be 50 % off
        torch.testing.assert_close(got[k].cpu().reshape(-1)[idx], ref32[k].reshape(-1)[idx], rtol=1e-5, atol=1e-9)
    assert float(got["stats"][7]) == float(ref32["stats"][7]) and float(got["stats"][9]) == float(ref32["stats"][9])


def run_loss(d, ticket=True, g_dtype=F32, dlp=True, dv=True, adv_stats=None, unbiased=1, c=0.2, cv=0.2, vf=1.0):
    """trlx_ppo_loss_elem (+ trlx_ppo_loss_finalize when ticket is False) with guarded outputs."""
    t = {k: cuda(d[k]).contiguous() for k in OPERANDS}
    n = t["lp"].numel()
    m = cuda(d["mask"])
    msum_host = float(n if m is None else int(d["mask"].sum()))
    nblk = _lib.query("trlx_ppo_loss_num_blocks", n)
    gl, gv = (Guarded(n, g_dtype) if dlp else None), (Guarded(n, g_dtype) if dv else None)
    part, loss, stats = Guarded(nblk * _lib.PPO_PARTIAL_SLOTS, torch.float64), Guarded(1, F32), Guarded(13, F32)
    tk = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = cuda(adv_stats)
    args = []
    for k in ("lp", "v", "olp", "ov", "adv"):
        args += [t[k].data_ptr(), _lib.dtype_code(t[k])]
    _lib.call("trlx_ppo_loss_elem", n, *args, _lib.ptr(st), unbiased, t["ret"].data_ptr(), _lib.dtype_code(t["ret"]),
              _lib.ptr(m), None, msum_host, c, cv, vf, None if gl is None else gl.ptr(), None if gv is None else gv.ptr(),
              _lib.dtype_code(torch.empty(0, dtype=g_dtype)), part.ptr(), loss.ptr() if ticket else None,
              stats.ptr() if ticket else None, tk.data_ptr() if ticket else None, stream())
    if not ticket:
        assert bool((loss.result() == SENTINEL).all()) and bool((stats.result() == SENTINEL).all())
        _lib.call("trlx_ppo_loss_finalize", part.ptr(), nblk, n, None, msum_host, vf, loss.ptr(), stats.ptr(), stream())
    out = dict(stats=stats.result(), loss=loss.result(), partials=part.result(), ticket=int(tk.cpu()))
    out["dlp"] = None if gl is None else gl.result(d["lp"].shape)
    out["dv"] = None if gv is None else gv.result(d["v"].shape)
    assert same_bits(out["loss"], out["stats"][:1])
    return out


@pytest.mark.parametrize("n", [513, 1061, 512 * 257 + 3])
def test_ppo_loss_c_abi_variants(n):
    d, ref32, want64 = loss_reference(n, 1, "random")
    full = run_loss(d)
    assert full["ticket"] == 0
    api = api_loss(d)
    for k in ("stats", "dlp", "dv"):
        assert same_bits(full[k], api[k].view_as(full[k])), k
    # the two-launch form: the same records summed in the same order
    two = run_loss(d, ticket=False)
    for k in ("stats", "loss", "partials", "dlp", "dv"):
        assert same_bits(two[k], full[k]), k
    # one gradient or the other left out
    no_dlp, no_dv = run_loss(d, dlp=False), run_loss(d, dv=False)
    assert same_bits(no_dlp["dv"], full["dv"]) and same_bits(no_dlp["stats"], full["stats"])
    assert same_bits(no_dv["dlp"], full["dlp"]) and same_bits(no_dv["stats"], full["stats"])
    # bf16 gradients
    g16 = run_loss(d, g_dtype=BF16)
    assert same_bits(g16["stats"], full["stats"])
    assert C.bf16_close(g16["dlp"], want64["dlp"]) and C.bf16_close(g16["dv"], want64["dv"])
    assert same_bits(g16["dlp"], full["dlp"].to(BF16)) and same_bits(g16["dv"], full["dv"].to(BF16))


@pytest.mark.parametrize("unbiased", [1, 0])
def test_ppo_loss_whitens_the_advantages_in_the_kernel(unbiased):
    n = 1061
    d, _, _ = loss_reference(n, 1, "random")
    m = C.moments64(d["adv"])
    st = torch.tensor([float(e) for e in m], dtype=torch.float64)
    got = run_loss(d, adv_stats=st, unbiased=unbiased)
    args = [d[k] for k in OPERANDS] + [d["mask"]]
    want64 = C.ppo_loss64(*args, adv_stats=m[:3], unbiased=bool(unbiased))
    ref32 = C.ppo_loss32(*args, adv_stats=m[:3], unbiased=bool(unbiased))
    check_rule(f"loss n={n} adv_stats unbiased={unbiased}", {k: got[k] for k in ("stats", "dlp", "dv")}, ref32, want64)


@pytest.mark.parametrize("masked_out", [False, True])
@pytest.mark.parametrize("operand", ["lp", "v", "ret"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_ppo_loss_non_finite_inputs_show_as_the_reference_shows_them(value, operand, masked_out):
    """torch.max and torch.clamp return NaN for a NaN operand: the loss and stats are NaN exactly
    where the reference's are (compare() gives inf otherwise), finite values keep the rule."""
    n = 513
    base, _, _ = loss_reference(n, 1, "random")
    d = {k: (None if t is None else t.clone()) for k, t in base.items()}
    flat_mask = d["mask"].view(-1)
    pos = int((flat_mask == (0 if masked_out else 1)).nonzero()[5])
    d[operand].view(-1)[pos] = value
    args = [d[k] for k in OPERANDS] + [d["mask"]]
    want64, ref32 = C.ppo_loss64(*args), C.ppo_loss32(*args)
    got = api_loss(d)
    check_rule(f"loss n={n} {operand}[{'masked' if masked_out else 'live'}]={value}", got, ref32, want64)
    for k in ("stats", "dlp", "dv"):
        assert torch.equal(torch.isnan(got[k].cpu().reshape(-1)), torch.isnan(want64[k].reshape(-1))), k
    if math.isnan(value) and operand in ("lp", "v"):
        assert math.isnan(float(got["stats"][0]))  # the loss itself is NaN, not a finite number


# ================================================================== k_scale_by alone
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("in_place", [True, False])
def test_scale_by(dtype, in_place):
    n = 8192 * 256 + 9  # one element-lap past the 8192 x 256 grid
    x = torch.randn(n, generator=C.gen(12)).to(dtype)
    for scale, want in ((1.0, x), (0.5, (x.float() * 0.5).to(dtype))):
        src = Guarded(n, dtype)
        src.view.copy_(x)
        dst = src if in_place else Guarded(n, dtype)
        s = torch.tensor([scale], dtype=F32, device=DEV)
        _lib.call("trlx_scale_by", src.ptr(), dst.ptr(), _lib.dtype_code(src.view), n, s.data_ptr(), stream())
        assert same_bits(dst.result(), want), scale  # 1: the buffer's bits; 0.5: exact
        if not in_place:
            assert same_bits(src.result(), x)
