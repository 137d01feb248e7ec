"""The oracle of the fused value head's tests: two restatements of make_head(n_embd, 1)
(trlx/model/nn/ppo_models.py:216-222) on the CPU.

  (a) reference_bf16   torch's own bf16 nn.Sequential (Linear, ReLU, Linear) and its bf16 autograd
  (b) oracle_fp64      the same function in fp64 with the ONE bf16 rounding of z = h·W1ᵀ + b1 that
                       a bf16 Linear applies; its autograd treats the rounding as the identity

The tests bound the kernel's distance to (b) by what (a) itself achieves:
    max|kernel − (b)| <= 2 · max|(a) − (b)| + 1e-6 · max|(b)|
(the factor 2: a different fp32 summation order may flip a bf16 rounding of z that torch's order
did not), for the values and for each of the five gradients.

The second half restates the kernel's walk over the 2H columns (csrc/value_head.hip k_vhead: S
contiguous slices in 32-column units, 128-column chunks, 32-deep K steps, z rounded to bf16 in
the chunk's epilogue) in plain torch, with a switch for the defects that only a workgroup with
several chunks can have.  tests/test_value_head_cpu.py shows that the rule above passes the
clean walk and rejects each defect; tests/test_gpu_value_head.py takes its shapes from here.
"""
import torch
from torch import nn

GRADS = ("dh", "dw1", "db1", "dw2", "db2")


def make_case(N, H, seed):
    """Seeded bf16 operands of a value head on N tokens, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16
    return dict(h=torch.randn(N, H, generator=g).to(bf),
                w1=(torch.randn(2 * H, H, generator=g) / H ** 0.5).to(bf),
                b1=(0.1 * torch.randn(2 * H, generator=g)).to(bf),
                w2=(torch.randn(1, 2 * H, generator=g) / (2 * H) ** 0.5).to(bf),
                b2=(0.1 * torch.randn(1, generator=g)).to(bf),
                dv=torch.randn(N, generator=g).to(bf))


def reference_module(w1, b1, w2, b2):
    """The reference's nn.Sequential with these parameters (names 0.weight, 0.bias, 2.weight, 2.bias)."""
    H = w1.shape[1]
    m = nn.Sequential(nn.Linear(H, 2 * H).bfloat16(), nn.ReLU().bfloat16(), nn.Linear(2 * H, 1).bfloat16())
    m.load_state_dict({"0.weight": w1, "0.bias": b1, "2.weight": w2.reshape(1, -1), "2.bias": b2.reshape(1)},
                      strict=True)
    return m


def reference_bf16(h, w1, b1, w2, b2, dv=None):
    """(a): values [N] bf16 and, with dv, the five gradients of torch's bf16 autograd."""
    m = reference_module(w1, b1, w2, b2)
    x = h.detach().clone().requires_grad_(dv is not None)
    out = m(x)
    res = {"values": out.detach().squeeze(-1)}
    if dv is not None:
        out.backward(dv.to(torch.bfloat16).reshape(out.shape))
        res.update(dh=x.grad, dw1=m[0].weight.grad, db1=m[0].bias.grad, dw2=m[2].weight.grad.reshape(-1),
                   db2=m[2].bias.grad.reshape(-1))
    return res


def round_bf16_ste(z):
    """bf16 rounding of an fp64 tensor whose gradient is the identity."""
    return z + (z.detach().float().to(torch.bfloat16).double() - z.detach())


def oracle_fp64(h, w1, b1, w2, b2, dv=None):
    """(b): values [N] fp64 and, with dv, the five fp64 gradients."""
    t = [x.detach().double().requires_grad_(dv is not None) for x in (h, w1, b1, w2.reshape(-1), b2.reshape(-1))]
    hd, w1d, b1d, w2d, b2d = t
    z = round_bf16_ste(hd @ w1d.t() + b1d)
    v = torch.relu(z) @ w2d + b2d
    res = {"values": v.detach()}
    if dv is not None:
        v.backward(dv.double().reshape(v.shape))
        res.update(dh=hd.grad, dw1=w1d.grad, db1=b1d.grad, dw2=w2d.grad, db2=b2d.grad)
    return res


def max_err(x, ref):
    return float((x.detach().double().cpu().reshape(-1) - ref.double().reshape(-1)).abs().max())


def bound(e_ref, ref):
    return 2.0 * e_ref + 1e-6 * float(ref.double().abs().max())


# ------------------------------------------------------------------ the kernel's column geometry
CHUNK, UNIT, KSTEP, TOKENS, HALF, MAX_SPLITS = 128, 32, 32, 64, 32, 64
MULTI_H = (96, 128, 256, 288, 320, 448, 768)   # nk mod 3 = 0, 1, 2, 0, 1, 2, 0; 2 .. 12 chunks at S = 1
FULL_N = (1, 33, 65, 130)
FULL_N_H = (256, 768)


def split_cap(H):
    return min(2 * H // UNIT, MAX_SPLITS)


def slices(H, S):
    """[c0, c1) of every column slice (vh_splits and k_vhead's c0 / c1)."""
    nu = 2 * H // UNIT
    S = max(1, min(S, split_cap(H)))
    return [((s * nu // S) * UNIT, ((s + 1) * nu // S) * UNIT) for s in range(S)]


def chunks(H, S):
    """128-column chunks each slice's workgroup walks."""
    return [-(-(c1 - c0) // CHUNK) for c0, c1 in slices(H, S)]


def multi_chunk_cases():
    """(N, H, S): every H of MULTI_H at the forced S in {1, 2, 3} that gives some workgroup two
    chunks or more, N = 65 everywhere and the full token list at H 256 and 768."""
    return [(N, H, S) for H in MULTI_H for S in (1, 2, 3) if max(chunks(H, S)) >= 2
            for N in (FULL_N if H in FULL_N_H else (65,))]


def case_seed(N, H):
    return 1000 * H + N


def one_hot_columns(H):
    """Columns for the one-hot w2 sweep: the first and last column of every chunk at S = 1 (the
    ragged last chunk's included) and 15 / 16 / 63 / 64 inside the second and the last chunk (the
    MFMA column groups' and the two column waves' edges)."""
    C = 2 * H
    cols = set()
    for c in range(0, C, CHUNK):
        cols.update((c, min(c + CHUNK, C) - 1))
    last = (C - 1) // CHUNK * CHUNK
    cols.update(c + k for c in (CHUNK, last) for k in (15, 16, 63, 64) if c + k < C)
    return sorted(cols)


DEFECTS = ("stale_vector", "stale_stage", "acc_kept", "unmasked", "empty_half")


def defect_reachable(defect, N, H, S):
    """Whether the (N, H, S) walk has the place where the defect acts."""
    if defect == "stale_vector":      # a b1 / w2 slot is used a second time: a fourth chunk
        return max(chunks(H, S)) >= 4
    if defect in ("stale_stage", "acc_kept"):
        return max(chunks(H, S)) >= 2
    if defect == "unmasked":          # a last chunk with columns at or past c1
        return any((c1 - c0) % CHUNK for c0, c1 in slices(H, S))
    if defect == "empty_half":        # the last token block's second 32 tokens hold none
        return (N - 1) % TOKENS < HALF
    raise ValueError(defect)


def chunked_walk(h, w1, b1, w2, b2, dv, S, defect=None):
    """k_vhead's walk in fp32 torch on the CPU: values [N] fp32 and the five bf16 gradients.

    defect (what a broken multi-chunk walk would compute):
      stale_vector  chunk c >= 3 takes the b1 / w2 of chunk c - 3 (the vector ring's slot reused
                    before its DMA landed)
      stale_stage   the middle K step of the second chunk of the first slice with two chunks
                    multiplies the h / W1 tile of three steps earlier (the stage ring's slot)
      acc_kept      the accumulator is not reset between chunks
      unmasked      the columns of a ragged chunk at or past c1 are not masked in the forward
                    (in the backward such a column below 2H rewrites what its own slice writes,
                    and one past 2H is a store outside dz that a restatement cannot hold)
      empty_half    a half block without a token leaves the previous half block's column sums
                    where zeros belong
    """
    assert defect is None or defect in DEFECTS
    N, H = h.shape
    C, nk = 2 * H, H // KSTEP
    hf, w1f, b1f, w2f, dvf = h.float(), w1.float(), b1.float(), w2.reshape(-1).float(), dv.reshape(-1).float()
    nhalf = 2 * (-(-N // TOKENS))
    half_of = torch.arange(N) // HALF
    dz = torch.zeros(N, C, dtype=torch.bfloat16)
    sw, sb = torch.zeros(nhalf, C), torch.zeros(nhalf, C)
    values = torch.zeros(N)
    lanes = torch.arange(CHUNK)
    stage_hit = False
    for c0, c1 in slices(H, S):
        nchunk = -(-(c1 - c0) // CHUNK)
        bad_step = -1
        if defect == "stale_stage" and nchunk >= 2 and not stage_hit:
            bad_step, stage_hit = nk + nk // 2, True
        acc = torch.zeros(N, CHUNK)
        part = torch.zeros(N)
        for ch in range(nchunk):
            for kt in range(nk):
                st = ch * nk + kt
                tch, tkt = divmod(st - 3, nk) if st == bad_step else (ch, kt)
                rows = (c0 + tch * CHUNK + lanes).clamp_max(C - 1)      # W1 rows clamped to the last one
                ks = slice(tkt * KSTEP, (tkt + 1) * KSTEP)
                acc = acc + hf[:, ks] @ w1f[rows, ks].t()
            col = c0 + ch * CHUNK + lanes
            ok = col < c1
            vch = ch - 3 if defect == "stale_vector" and ch >= 3 else ch
            vcol = c0 + vch * CHUNK + lanes
            vcol = torch.where(vcol < C, vcol, C - 2 + vcol % 2)        # the pair clamped to C - 2
            use = torch.ones_like(ok) if defect == "unmasked" else ok
            b1j = torch.where(use, b1f[vcol], torch.zeros(()))
            w2j = torch.where(use, w2f[vcol], torch.zeros(()))
            zb = (acc + b1j).to(torch.bfloat16).float()
            r = torch.relu(zb)
            part = part + (torch.where(use, r, torch.zeros(())) * w2j).sum(1)
            g = torch.where(zb > 0, (dvf[:, None] * w2j).to(torch.bfloat16).float(), torch.zeros(()))
            dz[:, col[ok]] = g[:, ok].to(torch.bfloat16)
            sw[:, col[ok]] = torch.zeros(nhalf, int(ok.sum())).index_add_(0, half_of, (dvf[:, None] * r)[:, ok])
            sb[:, col[ok]] = torch.zeros(nhalf, int(ok.sum())).index_add_(0, half_of, g[:, ok])
            if defect != "acc_kept":
                acc = torch.zeros(N, CHUNK)
        values = values + part
    values = values + b2.reshape(-1).float()
    if defect == "empty_half" and (N - 1) % TOKENS < HALF and nhalf >= 2:
        sw[-1], sb[-1] = sw[-2], sb[-2]
    dw2, db1 = torch.zeros(C), torch.zeros(C)
    for p in range(nhalf):     # k_vhead_bwd_reduce: the half blocks in order
        dw2, db1 = dw2 + sw[p], db1 + sb[p]
    bf = torch.bfloat16
    return dict(values=values, dh=(dz.float() @ w1f).to(bf), dw1=(dz.float().t() @ hf).to(bf), db1=db1.to(bf),
                dw2=dw2.to(bf), db2=dvf.sum().reshape(1).to(bf))


def over_the_bound(got, a, b):
    """The quantities of `got` that miss the rule against oracle b with torch's bf16 result a."""
    return [k for k in ("values",) + GRADS if not max_err(got[k], b[k]) <= bound(max_err(a[k], b[k]), b[k])]
