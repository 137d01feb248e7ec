"""GPU tests of the ILQL heads module (trlx-t5_amd/ilql_heads.py, csrc/ilql_heads.hip):
the target-Q heads evaluated at the action tokens only (trlx_ilql_tq_at_actions), the loss
on those gathered values (trlx_ilql_args.tq_gathered), the fused Polyak sync
(trlx_polyak_update) and ILQLHeads itself.

Tolerances
  gathered dot   |got - want| <= (K + 2)·2^-24·(Σ_k |z_k·w_k| + |b|) per element against the
                 fp64 value on the host: the standard bound of an fp32 dot of K products and a
                 bias in any summation order (bf16 inputs are quantised first; their products
                 are exact in fp32).
  loss           the gathered form hands the kernel the very fp32 value the full form loads,
                 so every output is compared bit for bit.
  Polyak         bit for bit against torch's own three ops, on the host and on the device.
                 IEEE 754 leaves the sign and payload of a NaN result open (x86 produces the
                 negative "default NaN", the GPU the positive one), so elements that are NaN
                 are compared as NaN and every other element by its bits.
  ILQLHeads      forward and hs gradients against an fp64 restatement at rtol 1e-5; atol 1e-5
                 covers outputs near zero (fp32 dots of <= 32 terms of magnitude ~1 carry an
                 absolute rounding error of up to ~32·2^-24·Σ|terms| ~ 1e-5).
"""
import pytest
import torch
import torch.nn.functional as F

import trlx_t5_amd as P
from trlx_t5_amd import _lib
from test_gpu_ilql import check, make_case, run_oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
FIELDS = ("input_ids", "attention_mask", "rewards", "states_ixs", "actions_ixs", "dones")


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_bits_or_nan(a, b):
    """Bitwise equality of every element that is not NaN; NaN where the other is NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


# ------------------------------------------------------------------ gathered dot
def a_star(ids, aix):
    return ids[:, 1:].gather(1, aix)


def dot_want(z, w, b, astar):
    """fp64 value and the fp32 dot bound (host tensors of the storage dtype)."""
    prod = z.double() * w.double()[astar]
    want, mag = prod.sum(-1), prod.abs().sum(-1)
    if b is not None:
        want = want + b.double()[astar]
        mag = mag + b.double()[astar].abs()
    return want, (z.shape[-1] + 2) * U * mag


def make_ids(B, A, V, g, mode="edges"):
    """input_ids [B, A+1] / actions_ixs [B, A] in the offline layout; a* covers 0 and V-1."""
    ids = torch.randint(0, V, (B, A + 1), generator=g)
    aix = torch.arange(A).repeat(B, 1)
    ids[0, 1] = 0
    ids[-1, -1] = V - 1
    if mode == "same":  # every row hits the same a*
        ids[:] = V // 2
    elif mode == "padded":  # pad_sequence zeros: a whole row of actions_ixs is 0
        aix[-1, :] = 0
    return ids, aix


def make_heads(B, A, K, V, dtype, nh, g, layout="plain", bias=True):
    """z [B, A, K], W2 [V, K], b2 [V] per head as host tensors (values) and device tensors in
    the requested layout: 'stride' = rows of K + 2 elements, 'offset' = z one element into its
    storage."""
    host, dev = [], []
    for _ in range(nh):
        z = torch.relu(torch.randn(B, A, K, generator=g)).to(dtype)
        w = (torch.randn(V, K, generator=g) / max(1.0, K ** 0.5)).to(dtype)
        b = torch.randn(V, generator=g).to(dtype) if bias else None
        host.append((z, w, b))
        if layout == "stride":
            zb = torch.zeros(B, A, K + 2, dtype=dtype, device=DEV)
            wb = torch.zeros(V, K + 2, dtype=dtype, device=DEV)
            zb[..., :K] = z.to(DEV)
            wb[:, :K] = w.to(DEV)
            zd, wd = zb[..., :K], wb[:, :K]
            assert zd.stride(1) == K + 2 and wd.stride(0) == K + 2
        elif layout == "offset":
            flat = torch.zeros(B * A * K + 1, dtype=dtype, device=DEV)
            flat[1:] = z.to(DEV).reshape(-1)
            zd, wd = flat[1:].view(B, A, K), w.to(DEV)
            assert (zd.data_ptr() - flat.data_ptr()) == z.element_size()
        else:
            zd, wd = z.to(DEV), w.to(DEV)
        dev.append((zd, wd, None if b is None else b.to(DEV)))
    return host, dev


def run_dot(dev, ids, aix):
    outs = P.ilql_target_q_at_actions([d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev],
                                      ids.to(DEV), aix.to(DEV))
    torch.cuda.synchronize()
    assert len(outs) == len(dev)
    return [o.cpu() for o in outs]


def check_dot(outs, host, ids, aix):
    astar = a_star(ids, aix)
    for o, (z, w, b) in zip(outs, host):
        assert o.dtype == torch.float32 and tuple(o.shape) == tuple(astar.shape)
        want, bound = dot_want(z, w, b, astar)
        err = (o.double() - want).abs()
        print("max err / bound", float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (err.max(), bound.min())


DOT_SHAPES = [  # B, A, K, V, layout, bias
    (2, 3, 6, 37, "plain", True),
    (3, 5, 1536, 211, "plain", True),
    (1, 2, 1, 5, "plain", True),       # K = 1; A != 1 while B == 1
    (2, 3, 257, 11, "stride", True),   # row stride 259 elements: rows off the 16-B grid
    (2, 3, 16, 11, "stride", True),    # K a vector multiple, stride 18: aligned and unaligned rows mix
    (2, 3, 8, 13, "offset", True),     # z starts one element into its storage
    (2, 3, 12, 17, "plain", False),    # b2 = None
]


@pytest.mark.parametrize("nh", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,A,K,V,layout,bias", DOT_SHAPES)
def test_tq_at_actions_vs_fp64(B, A, K, V, layout, bias, dtype, nh):
    g = torch.Generator().manual_seed(11 * K + V + nh)
    ids, aix = make_ids(B, A, V, g)
    host, dev = make_heads(B, A, K, V, dtype, nh, g, layout, bias)
    astar = a_star(ids, aix)
    assert int(astar.min()) == 0 and int(astar.max()) == V - 1
    outs = run_dot(dev, ids, aix)
    check_dot(outs, host, ids, aix)
    if layout != "plain":  # the summation order is fixed by (K, dtype): alignment changes no bit
        plain = run_dot([(z.to(DEV), w.to(DEV), None if b is None else b.to(DEV)) for z, w, b in host], ids, aix)
        for o, p in zip(outs, plain):
            assert same_bits(o, p)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["same", "padded"])
def test_tq_at_actions_repeated_tokens(mode, dtype):
    B, A, K, V = 3, 4, 40, 29
    g = torch.Generator().manual_seed(5)
    ids, aix = make_ids(B, A, V, g, mode)
    if mode == "same":
        assert int(a_star(ids, aix).min()) == int(a_star(ids, aix).max())
    else:
        assert int(aix[-1].abs().sum()) == 0
    host, dev = make_heads(B, A, K, V, dtype, 2, g)
    check_dot(run_dot(dev, ids, aix), host, ids, aix)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tq_at_actions_out_of_range_token_is_nan(dtype):
    """a* = V (through input_ids) gives NaN in that element only, its neighbours unchanged;
    an actions_ixs entry outside [0, L-1) likewise (as y_ok in the loss)."""
    B, A, K, V = 2, 4, 24, 19
    g = torch.Generator().manual_seed(6)
    ids, aix = make_ids(B, A, V, g)
    host, dev = make_heads(B, A, K, V, dtype, 2, g)
    clean = run_dot(dev, ids, aix)
    bad_ids = ids.clone()
    bad_ids[1, 1 + 2] = V
    bad_aix = aix.clone()
    bad_aix[0, 1] = A  # = L - 1: outside [0, L-1)
    for got, hit in ((run_dot(dev, bad_ids, aix), (1, 2)), (run_dot(dev, ids, bad_aix), (0, 1))):
        for o, c in zip(got, clean):
            mask = torch.zeros(B, A, dtype=torch.bool)
            mask[hit] = True
            assert torch.equal(torch.isnan(o), mask)
            assert torch.equal(bits(o)[~mask], bits(c)[~mask])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tq_at_actions_reproducible_and_batch_independent(dtype):
    """Two calls agree bit for bit, and a (b, a) output keeps its bits when the same rows sit
    inside a larger batch (another grid, other workgroups)."""
    B, A, K, V = 3, 5, 1536, 211
    g = torch.Generator().manual_seed(8)
    ids, aix = make_ids(B, A, V, g)
    host, dev = make_heads(B, A, K, V, dtype, 2, g)
    first, second = run_dot(dev, ids, aix), run_dot(dev, ids, aix)
    for a, b in zip(first, second):
        assert same_bits(a, b)
    ids2, aix2 = make_ids(4, A, V, g)
    _, dev2 = make_heads(4, A, K, V, dtype, 2, g)
    big_ids = torch.cat([ids2[:3], ids, ids2[3:]])
    big_aix = torch.cat([aix2[:3], aix, aix2[3:]])
    big = [(torch.cat([d2[0][:3], d[0], d2[0][3:]]), d[1], d[2]) for d, d2 in zip(dev, dev2)]
    for a, b in zip(first, run_dot(big, big_ids, big_aix)):
        assert same_bits(a, b[3:3 + B])


def test_tq_at_actions_refuses_bad_arguments():
    g = torch.Generator().manual_seed(9)
    ids, aix = make_ids(2, 3, 7, g)
    _, dev = make_heads(2, 3, 4, 7, torch.float32, 1, g)
    z, w, b = dev[0]
    with pytest.raises(ValueError):
        P.ilql_target_q_at_actions([z], [w[:, :3]], [b], ids.to(DEV), aix.to(DEV))
    with pytest.raises(TypeError):
        P.ilql_target_q_at_actions([z], [w.bfloat16()], [b], ids.to(DEV), aix.to(DEV))
    with pytest.raises(ValueError):
        P.ilql_target_q_at_actions([z], [w], [b], ids.to(DEV), aix[:, :2].to(DEV))


# ------------------------------------------------------------------ loss on gathered target Q
def dev_batch(b):
    return P.ILQLBatch(*(getattr(b, f).to(DEV) for f in FIELDS))


def loss_forms(B, L, V, nq, seed, nan=False):
    """A loss case with the target heads in both forms: random T_i [B, A] fp32, and full
    [B, A, V] noise tensors with T_i scattered at a*."""
    logits, qs, _, vs, b = make_case(B, L, V, seed, nq=nq)
    g = torch.Generator().manual_seed(seed + 1)
    A = L - 1
    astar = a_star(b.input_ids, b.actions_ixs)
    Ts = [torch.randn(B, A, generator=g) for _ in range(nq)]
    if nan:
        Ts[0][0, 0] = float("nan")
    full = [torch.randn(B, A, V, generator=g).scatter_(-1, astar[..., None], T[..., None]) for T in Ts]
    return logits, qs, vs, b, Ts, full


def run_loss(cfg, logits, qs, tqs, vs, bd):
    lg = logits.to(DEV).requires_grad_(True)
    q = [x.to(DEV).requires_grad_(True) for x in qs]
    v = vs.to(DEV).requires_grad_(True)
    loss, stats = cfg.loss((lg, (q, [t.to(DEV) for t in tqs], v)), bd)
    loss.backward()
    torch.cuda.synchronize()
    return [loss.detach()] + [stats[k].detach() for k in P.ILQL_LOSS_KEYS] + [lg.grad] + [x.grad for x in q] + [v.grad]


@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("B,L,V", [(3, 6, 37), (2, 5, 50257)])
def test_loss_on_gathered_target_q_is_exact(B, L, V, nq):
    logits, qs, vs, b, Ts, full = loss_forms(B, L, V, nq, 40 + V + nq)
    cfg = P.ILQLConfig(two_qs=nq == 2)
    bd = dev_batch(b)
    want = run_loss(cfg, logits, qs, full, vs, bd)
    for form in (Ts, [T[..., None] for T in Ts]):  # [B, A] and [B, A, 1]
        got = run_loss(cfg, logits, qs, form, vs, bd)
        assert len(got) == len(want) == 1 + 5 + 1 + nq + 1
        for a, w in zip(got, want):
            assert torch.equal(a, w) and same_bits(a, w)
    # the pair is anchored to the oracle through the full form (test_gpu_ilql.py tolerances)
    gl = want[0].cpu()
    stats = dict(zip(P.ILQL_LOSS_KEYS, (s.cpu() for s in want[1:6])))
    check((gl, {k: stats[f"losses/{k}"] for k in ("loss", "loss_q", "loss_v", "loss_cql", "loss_awac")},
           want[6].cpu(), [x.cpu() for x in want[7:7 + nq]], want[7 + nq].cpu()),
          run_oracle(logits, qs, full, vs, b))


@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("B,L,V", [(3, 6, 37), (2, 5, 50257)])
def test_hot_path_on_gathered_target_q_is_exact(B, L, V, nq):
    logits, qs, vs, b, Ts, full = loss_forms(B, L, V, nq, 60 + V + nq)
    cfg = P.ILQLConfig(two_qs=nq == 2)
    hp = P.ILQLHotPath(cfg, B, L, V, torch.float32, DEV)
    bd = dev_batch(b)
    lg, q, v = logits.to(DEV), [x.to(DEV) for x in qs], vs.to(DEV).reshape(B, L)

    def step(tqs):
        losses, dl, dq, dvs = hp.step(lg, q, [t.to(DEV) for t in tqs], v, bd)
        torch.cuda.synchronize()
        return [losses.clone(), dl.clone()] + [x.clone() for x in dq] + [dvs.clone()]

    want = step(full)
    for form in (Ts, [T[..., None] for T in Ts]):
        for a, w in zip(step(form), want):
            assert torch.equal(a, w) and same_bits(a, w)
    with pytest.raises(ValueError):
        step([full[0]] + Ts[1:] if nq == 2 else [Ts[0].double()])
    with pytest.raises(ValueError):
        step([T.bfloat16() for T in Ts])


def test_gathered_nan_propagates_as_in_the_full_form():
    B, L, V = 3, 6, 37
    logits, qs, vs, b, Ts, full = loss_forms(B, L, V, 2, 77, nan=True)
    b.dones[:] = 1  # the NaN row carries weight
    b.dones[:, -1] = 0
    b.attention_mask[:] = 1
    cfg = P.ILQLConfig()
    bd = dev_batch(b)
    want, got = run_loss(cfg, logits, qs, full, vs, bd), run_loss(cfg, logits, qs, Ts, vs, bd)
    assert bool(torch.isnan(want[0])) and bool(torch.isnan(want[-1]).any())
    for a, w in zip(got, want):
        assert same_bits(a, w)


def test_mixed_target_q_forms_raise():
    B, L, V = 3, 6, 37
    logits, qs, vs, b, Ts, full = loss_forms(B, L, V, 2, 78)
    bd = dev_batch(b)
    args = [x.to(DEV) for x in (logits, vs)]
    q = [x.to(DEV) for x in qs]
    for tqs in ([full[0], Ts[1]], [Ts[0], full[1]]):
        with pytest.raises(ValueError, match="mixes"):
            P.ILQLConfig().loss((args[0], (q, [t.to(DEV) for t in tqs], args[1])), bd)
    with pytest.raises(ValueError):
        P.ILQLConfig().loss((args[0], (q, [T[:, :-1].to(DEV) for T in Ts], args[1])), bd)


# ------------------------------------------------------------------ Polyak update
SPECIALS = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1e-40, -1e-40, 2e-38, 1.5]
SIZES = [1, 7, 1536, 2 * 1536 + 3, 0]


def polyak_tensors(sizes, dtype, g):
    """(sources, targets) on the host; tensors of >= 81 elements start with every pair of
    SPECIALS (±0, ±inf, NaN, denormals, a product that goes denormal)."""
    S, T = [], []
    sp = torch.tensor(SPECIALS)
    for n in sizes:
        s, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
        if n >= len(SPECIALS) ** 2:
            s[:len(sp) ** 2] = sp.repeat_interleave(len(sp))
            t[:len(sp) ** 2] = sp.repeat(len(sp))
        elif n >= len(sp):
            s[:len(sp)] = sp
        S.append(s.to(dtype))
        T.append(t.to(dtype))
    return S, T


def to_dev(ts, offset=0):
    """Device copies; offset: each tensor is a view starting `offset` elements into its storage."""
    out = []
    for t in ts:
        buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=DEV)
        buf[offset:] = t.to(DEV)
        out.append(buf[offset:])
    return out


def torch_polyak(t, s, alpha):
    t = t.clone()
    t.copy_((alpha * s) + (1.0 - alpha) * t)
    return t


def check_polyak(S, T, alpha, target_offset=0, source_offset=0):
    sd, td = to_dev(S, source_offset), to_dev(T, target_offset)
    for t in td:
        assert t.numel() == 0 or (t.data_ptr() % 16) == (target_offset * t.element_size()) % 16
    want_dev = [torch_polyak(t, s, alpha) for t, s in zip(td, sd)]
    want_host = [torch_polyak(t, s, alpha) for t, s in zip(T, S)]
    P.polyak_update(td, sd, alpha)
    torch.cuda.synchronize()
    for i, (got, wd, wh, s0, s1) in enumerate(zip(td, want_dev, want_host, S, sd)):
        assert same_bits_or_nan(got, wd), f"tensor {i} ({got.numel()} elements) vs torch on the device"
        assert same_bits_or_nan(got, wh), f"tensor {i} ({got.numel()} elements) vs torch on the host"
        assert same_bits(s1.cpu(), s0), f"source {i} changed"


@pytest.mark.parametrize("alpha", [0.001, 0.0, 1.0, 0.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_polyak_update_matches_torch_bitwise(dtype, alpha):
    g = torch.Generator().manual_seed(21)
    S, T = polyak_tensors(SIZES, dtype, g)
    assert any(bool(torch.isnan(t).any()) for t in T) and any(bool(torch.isinf(s).any()) for s in S)
    check_polyak(S, T, alpha)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("target_offset,source_offset", [(1, 0), (1, 1), (0, 3)])
def test_polyak_update_views_off_the_vector_grid(target_offset, source_offset, dtype):
    """A target (or source) starting one element into its storage: the pair's 16-B phases
    differ (element path) or agree (head / body / tail path).  20005 elements: several
    workgroups per tensor."""
    g = torch.Generator().manual_seed(22)
    S, T = polyak_tensors(SIZES + [20005], dtype, g)
    check_polyak(S, T, 0.3, target_offset, source_offset)


def test_polyak_update_list_longer_than_the_table():
    n = _lib.POLYAK_MAX_TENSORS + 1
    g = torch.Generator().manual_seed(23)
    S, T = polyak_tensors([3 + 5 * i for i in range(n)], torch.float32, g)
    check_polyak(S, T, 0.001)
    # fp32 and bf16 pairs in one call: grouped by dtype
    Sb, Tb = polyak_tensors([9, 100], torch.bfloat16, g)
    check_polyak(S[:2] + Sb + S[2:4], T[:2] + Tb + T[2:4], 0.3)


def test_polyak_update_refuses_aliasing_and_mismatches():
    t = torch.randn(64, device=DEV)
    keep = t.clone()
    with pytest.raises(ValueError, match="alias"):
        P.polyak_update([t], [t], 0.5)
    with pytest.raises(ValueError, match="alias"):
        P.polyak_update([t[:40]], [t[8:48]], 0.5)
    first = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError, match="alias"):  # refused before anything is launched
        P.polyak_update([first, t], [torch.ones(4, device=DEV), t], 0.5)
    torch.cuda.synchronize()
    assert torch.equal(t, keep) and float(first.abs().sum()) == 0.0
    with pytest.raises(ValueError):
        P.polyak_update([t], [t.clone().bfloat16()], 0.5)
    with pytest.raises(ValueError):
        P.polyak_update([t], [torch.randn(65, device=DEV)], 0.5)
    with pytest.raises(ValueError):
        P.polyak_update([t], [], 0.5)


# ------------------------------------------------------------------ ILQLHeads
def heads_case(two_qs, padded, seed=31):
    H, V, B, L = 16, 37, 3, 7
    torch.manual_seed(seed)
    heads = P.ILQLHeads(P.ILQLConfig(two_qs=two_qs), H, V).to(DEV)
    with torch.no_grad():  # the targets are a deepcopy of the Q heads: make them differ
        for p in heads.target_q_heads.parameters():
            p.add_(0.05 * torch.randn_like(p))
    g = torch.Generator().manual_seed(seed)
    hs = torch.randn(B, L, H, generator=g)
    ids = torch.randint(0, V, (B, L), generator=g)
    six, aix = torch.arange(L).repeat(B, 1), torch.arange(L - 1).repeat(B, 1)
    if padded:  # pad_sequence zeros: repeated index 0
        six[-1, 3:] = 0
        aix[-1, 2:] = 0
        six[1, 5:] = 0
        aix[1, 4:] = 0
    return heads, hs, ids, six, aix


def head64(seq, x):
    w = [p.detach().cpu().double() for p in seq.parameters()]
    return F.linear(torch.relu(F.linear(x, w[0], w[1])), w[2], w[3])


def restate64(heads, hs, six, aix):
    """The reference's forward in fp64: hs.gather with the repeated index, Linear, ReLU, Linear."""
    H = hs.shape[-1]
    s_hs = hs.gather(1, six.unsqueeze(-1).repeat(1, 1, H))
    a_hs = hs.gather(1, aix.unsqueeze(-1).repeat(1, 1, H))
    return (tuple(head64(h, a_hs) for h in heads.q_heads), tuple(head64(h, a_hs) for h in heads.target_q_heads),
            head64(heads.v_head, s_hs))


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("two_qs", [True, False])
def test_heads_forward_and_hs_gradient_vs_fp64(two_qs, padded):
    heads, hs, ids, six, aix = heads_case(two_qs, padded)
    tol = dict(rtol=1e-5, atol=1e-5)
    hd = hs.to(DEV).requires_grad_(True)
    qs, tqs, vs = heads(hd, six.to(DEV), aix.to(DEV))
    h64 = hs.double().requires_grad_(True)
    wq, wtq, wvs = restate64(heads, h64, six, aix)
    assert len(qs) == len(tqs) == (2 if two_qs else 1)
    for got, want in zip(qs + tqs + (vs,), wq + wtq + (wvs,)):
        assert got.dtype == torch.float32 and got.shape == want.shape
        torch.testing.assert_close(got.detach().cpu().double(), want.detach(), **tol)
    assert all(q.requires_grad for q in qs)  # (the full target rows carry hs's graph, as the reference's do)
    g = torch.Generator().manual_seed(3)
    cq = [torch.randn(q.shape, generator=g) for q in qs]
    cv = torch.randn(vs.shape, generator=g)
    (sum((q * c.to(DEV)).sum() for q, c in zip(qs, cq)) + (vs * cv.to(DEV)).sum()).backward()
    (sum((q * c.double()).sum() for q, c in zip(wq, cq)) + (wvs * cv.double()).sum()).backward()
    torch.testing.assert_close(hd.grad.cpu().double(), h64.grad, **tol)
    # without indices the heads run on every position
    q_all, _, v_all = heads(hs.to(DEV))
    assert tuple(q_all[0].shape) == (3, 7, 37) and tuple(v_all.shape) == (3, 7, 1)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("two_qs", [True, False])
def test_heads_forward_for_loss(two_qs, padded):
    heads, hs, ids, six, aix = heads_case(two_qs, padded)
    B, L, V = 3, 7, 37
    hd = hs.to(DEV).requires_grad_(True)
    idd, sd, ad = ids.to(DEV), six.to(DEV), aix.to(DEV)
    qs, tq_at, vs = heads.forward_for_loss(hd, idd, sd, ad)
    _, tq_full, vs_full = heads(hd, sd, ad)
    astar = a_star(ids, aix)
    rows = torch.arange(B, device=DEV)[:, None]
    for t, full, seq in zip(tq_at, tq_full, heads.target_q_heads):
        assert tuple(t.shape) == (B, L - 1) and t.dtype == torch.float32 and not t.requires_grad
        with torch.no_grad():
            z = seq[1](seq[0](hd[rows, ad]))
        want, bound = dot_want(z.cpu(), seq[2].weight.detach().cpu(), seq[2].bias.detach().cpu(), astar)
        assert bool(((t.cpu().double() - want).abs() <= bound).all())
        gathered = full.gather(-1, astar.to(DEV)[..., None]).squeeze(-1).cpu().double()
        assert bool(((t.cpu().double() - gathered).abs() <= bound).all())
    assert same_bits(vs, vs_full)
    # end to end: the loss takes the gathered targets, gradients reach hs and the trainable heads
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(B, L, V, generator=g).to(DEV).requires_grad_(True)
    dones = torch.ones(B, L, dtype=torch.long)
    dones[:, -1] = 0
    batch = P.ILQLBatch(idd, torch.ones(B, L, dtype=torch.long, device=DEV), torch.randn(B, L - 1, generator=g).to(DEV),
                        sd, ad, dones.to(DEV))
    loss, stats = heads.config.loss((logits, (qs, tq_at, vs)), batch)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and list(stats) == list(P.ILQL_LOSS_KEYS)
    assert hd.grad is not None and bool(torch.isfinite(hd.grad).all()) and float(hd.grad.abs().sum()) > 0
    assert all(p.grad is not None for p in heads.q_heads.parameters())
    assert all(p.grad is not None for p in heads.v_head.parameters())
    assert all(p.grad is None for p in heads.target_q_heads.parameters())
    # and equals the loss on the full target rows
    loss_full, _ = heads.config.loss((logits, (qs, [t.detach() for t in tq_full], vs)), batch)
    torch.testing.assert_close(loss.detach(), loss_full.detach(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("two_qs", [True, False])
def test_heads_sync_target_q_heads(two_qs):
    heads, *_ = heads_case(two_qs, False)
    alpha = heads.config.alpha
    q_before = [p.detach().clone() for p in heads.q_heads.parameters()]
    want = [torch_polyak(t.detach(), q.detach(), alpha)
            for t, q in zip(heads.target_q_heads.parameters(), heads.q_heads.parameters())]
    before = [t.detach().clone() for t in heads.target_q_heads.parameters()]
    heads.sync_target_q_heads()
    torch.cuda.synchronize()
    assert len(want) == (8 if two_qs else 4)
    for t, w, b0 in zip(heads.target_q_heads.parameters(), want, before):
        assert same_bits(t.detach(), w) and not t.requires_grad
        assert not torch.equal(t.detach(), b0)
    for q, q0 in zip(heads.q_heads.parameters(), q_before):
        assert same_bits(q.detach(), q0) and q.requires_grad
