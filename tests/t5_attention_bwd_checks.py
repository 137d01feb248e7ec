"""The gradient side of tests/t5_attention_checks.py for T5's full-sequence attention backward
(csrc/t5_attention_bwd.hip, t5_attention_train): the float64 gradient oracle, torch's own bf16
autograd as the yardstick, the shared sizes and the rule.

oracle_grads    torch.autograd.grad through C.oracle in float64, on the bf16-rounded q, k, v and a
                seeded N(0, 1) dO rounded to bf16; the bias goes in as a float64 [nH, Tq + S - 1]
                table leaf built from W by offset, so its gradient is the bias TABLE's.
eager_grads     autograd through C.eager in bf16 on the tensors' device (HF's op order), the table
                an fp32 leaf.
The rule, per gradient g in {dq, dk, dv, dbias}:
    max|g_kernel - g_oracle| <= 2 * max|g_eager - g_oracle| + one bf16 ulp of max|g_oracle|
The factor 2 as in the forward: the kernels round P and dS to bf16 as MFMA operands, as torch rounds
them, but un-normalised and summed in another order.
"""
import contextlib

import torch

import t5_attention_checks as C
from t5_attention_checks import case, make_mask, poison, oracle, eager, bucket, bf16_ulp, bound  # noqa: F401

GRADS = ("dq", "dk", "dv", "dbias")


def sizes(tile_pairs):
    """C.sizes over every (row tile, column tile) pair of the forward and the backward kernels."""
    return sorted(set().union(*(C.sizes(a, b) for a, b in tile_pairs)))


def cross_sizes(tile_pairs):
    out = []
    for a, b in tile_pairs:
        out += [p for p in C.cross_sizes(a, b) if p not in out]
    return out


def bucket_index(Tq, S, bidirectional):
    """int64 [Tq + S - 1]: C.bucket(j - i) by offset (j - i) + Tq - 1."""
    return torch.tensor([C.bucket(o, bidirectional) for o in range(-(Tq - 1), S)])


def table_from(W, Tq, S, bidirectional, dtype=torch.float64):
    """[nH, Tq + S - 1] from W [num_buckets, nH]."""
    return W.to(dtype)[bucket_index(Tq, S, bidirectional)].t().contiguous()


def make_dout(d_kv, Tq, S, seed=0, Bc=C.B, nH=C.NH):
    g = torch.Generator().manual_seed(77000 + 131 * Tq + 17 * S + d_kv + 100003 * seed)
    return torch.randn(Bc, Tq, nH * d_kv, generator=g).to(torch.bfloat16)


@contextlib.contextmanager
def _bias_from_table(table):
    """C.oracle adds C.oracle_bias(weight, ...), looked up as a global of its module at call time: for
    this block that name is `table` looked up by offset (shift moves every offset, as C.oracle's
    bias_shift asks; the ends repeat).  Serial use only; yields the list of calls made, which
    oracle_grads checks, so a C.oracle that binds the function some other way fails loudly."""
    calls = []

    def by_offset(weight, Tq, S, bidirectional, shift=0):
        calls.append((Tq, S))
        rel = torch.arange(S)[None, :] - torch.arange(Tq)[:, None] + shift
        return table[:, (rel + (Tq - 1)).clamp(0, Tq + S - 2)]
    keep = C.oracle_bias
    C.oracle_bias = by_offset
    try:
        yield calls
    finally:
        C.oracle_bias = keep


def oracle_grads(q, k, v, dout, table=None, mask=None, causal=False, drop_delta=False, per_batch_dbias=False, **wrong):
    """out and the gradients in float64.  q [B, nH, Tq, d], k / v [B, nH, S, d] (any values in the
    masked rows: C.oracle does not read them), dout [B, Tq, nH*d], table float64 [nH, Tq + S - 1] or
    None.  `wrong` goes to C.oracle (bias_shift, drop_key, causal_shift); drop_delta leaves the
    `delta` term out of dS; per_batch_dbias returns batch row 0's dbias without the sum over b."""
    q, k, v = (x.detach().double().nan_to_num(0.0).requires_grad_() for x in (q, k, v))
    leaves = [q, k, v]
    if table is not None:
        table = table.detach().double().requires_grad_()
        leaves.append(table)
    with _bias_from_table(table) as calls:
        out = C.oracle(q, k, v, table, True, mask=mask, causal=causal, **wrong)
    # C.oracle has to have taken its bias through the module-level name swapped above
    assert len(calls) == (0 if table is None else 1), "C.oracle no longer looks oracle_bias up in its module"
    g = dout.double()
    if drop_delta:
        # dS = P dP instead of P (dP - delta): the softmax's own backward term is lost.  Rebuild it:
        # d out / d s through a softmax whose normaliser is treated as a constant.
        Bq, nH, Tq, d = q.shape
        live = torch.ones(Bq, Tq, k.shape[2], dtype=torch.bool)
        if mask is not None:
            live &= (mask != 0)[:, None, :]
        if causal:
            live &= (torch.arange(k.shape[2])[None, :] <= torch.arange(Tq)[:, None])[None]
        kk = k.masked_fill(~live.any(1)[:, None, :, None], 0.0)
        vv = v.masked_fill(~live.any(1)[:, None, :, None], 0.0)
        s = torch.einsum("bhid,bhjd->bhij", q, kk)
        if table is not None:
            rel = torch.arange(k.shape[2])[None, :] - torch.arange(Tq)[:, None]
            s = s + table[:, rel + Tq - 1][None]
        s = s.masked_fill(~live[:, None], float("-inf"))
        z = torch.logsumexp(s, dim=-1, keepdim=True).detach()
        p = torch.exp(s - z)
        out2 = torch.einsum("bhij,bhjd->bihd", p, vv).reshape(out.shape)
        grads = torch.autograd.grad(out2, leaves, g)
    else:
        grads = torch.autograd.grad(out, leaves, g)
    res = dict(out=out.detach(), dq=grads[0], dk=grads[1], dv=grads[2], dbias=grads[3] if table is not None else None)
    if per_batch_dbias and table is not None:
        one = oracle_grads(q[:1], k[:1], v[:1], dout[:1], table, None if mask is None else mask[:1], causal)
        res["dbias"] = one["dbias"]
    return res


def eager_grads(q, k, v, dout, table=None, mask=None, causal=False):
    """The yardstick: autograd through C.eager in the tensors' dtype on their device; k, v finite in
    the masked rows; table an fp32 [nH, Tq + S - 1] or None."""
    q, k, v = (x.detach().clone().requires_grad_() for x in (q, k, v))
    leaves = [q, k, v]
    if table is not None:
        table = table.detach().float().clone().requires_grad_()
        leaves.append(table)
    out = C.eager(q, k, v, table, mask, causal)
    grads = torch.autograd.grad(out, leaves, dout.to(out.dtype))
    return dict(out=out.detach(), dq=grads[0], dk=grads[1], dv=grads[2], dbias=grads[3] if table is not None else None)


def max_err(x, ref):
    return C.max_err(x, ref)


def judge(got, yard, want):
    """Per gradient: (e_kernel, e_torch, bound).  `got`, `yard`, `want`: dicts as oracle_grads returns."""
    out = {}
    for n in GRADS:
        if want.get(n) is None:
            continue
        e_k, e_t = max_err(got[n], want[n]), max_err(yard[n], want[n])
        out[n] = (e_k, e_t, C.bound(e_t, want[n]))
    return out
