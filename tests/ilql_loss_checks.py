"""Shared pieces of the ILQL loss tests (csrc/ilql_rows.hip: k_ilql_prep, k_ilql_rows,
k_ilql_finalize; used by tests/test_gpu_ilql.py, tests/test_gpu_ilql_edges.py and the CPU file
tests/test_ilql_loss_table.py).

  run_gpu / run_oracle / check / make_case   the drop-in route (ILQLConfig.loss with autograd)
                against the fp32 oracle, as tests/test_gpu_ilql.py has always used them
  oracle64 / check64   oracle.ppo_oracle.ilql_loss on .double() inputs with its autograd, and the
                project's fp32 bar against it (fp32 rows rtol 1e-5 / atol 1e-6; bf16 rows
                rtol 1e-2 / atol 2e-6 on the row gradients only)
  select / entry_of / TABLE_V ...   the launch table of trlx_ilql_rows restated:
                (dtype, V, split_lds, ilql_split) -> (path, NV, NL, threads)
  row_split / locate / y_positions   common.h RowSplit and line_shift restated: which head / tail
                element or which (vector, lane, step) of the kernel holds element j of a row
  phased / launch   rows placed at chosen 16-B and 256-B phases inside a wider filled buffer, and
                one trlx_ilql_* call on device tensors as they are (gradient buffers filled with
                FILL first, so an element the kernel does not write keeps it)
  CASES         every input set of the edge suite by name; the CPU file proves for each that the
                fp32 oracle itself stays inside the bar against the fp64 oracle

Test infrastructure only."""
import ctypes
import functools

import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
from trlx_t5_amd.modeling import grad_buffer_like
from oracle import ppo_oracle as orc

DEV = torch.device("cuda:0")
KEYS = ("loss", "loss_q", "loss_v", "loss_cql", "loss_awac")
FIELDS = ("input_ids", "attention_mask", "rewards", "states_ixs", "actions_ixs", "dones")
FILL = 7.0           # exactly representable in bf16; no gradient of these cases equals it
ERR_SHAPE, ERR_STRIDE = 1, 2
F32, BF16 = torch.float32, torch.bfloat16


# ------------------------------------------------------------------ the drop-in route, fp32 oracle
def run_gpu(cfg, logits, qs, tqs, vs, batch, grad_scale=1.0):
    lg = logits.to(DEV).requires_grad_(True)
    q = [x.to(DEV).requires_grad_(True) for x in qs]
    tq = [x.to(DEV) for x in tqs]
    v = vs.to(DEV).requires_grad_(True)
    b = P.ILQLBatch(*(getattr(batch, f).to(DEV) for f in FIELDS))
    loss, stats = cfg.loss((lg, (q, tq, v)), b)
    assert list(stats) == [f"losses/{k}" for k in ("loss_q", "loss_v", "loss_cql", "loss_awac", "loss")]
    (loss * grad_scale).backward()
    torch.cuda.synchronize()
    return (loss.detach().cpu(), {k: stats[f"losses/{k}"].detach().cpu() for k in KEYS}, lg.grad.cpu(),
            [x.grad.cpu() for x in q], v.grad.cpu())


def run_oracle(logits, qs, tqs, vs, batch, grad_scale=1.0, **kw):
    lg = logits.float().requires_grad_(True)
    q = [x.float().requires_grad_(True) for x in qs]
    v = vs.float().requires_grad_(True)
    loss, stats = orc.ilql_loss(lg, q, [x.float() for x in tqs], v, batch.input_ids, batch.attention_mask,
                                batch.rewards, batch.actions_ixs, batch.dones, **kw)
    (loss * grad_scale).backward()
    return (loss.detach(), {k: stats[f"losses/{k}"].detach() for k in KEYS}, lg.grad, [x.grad for x in q],
            v.grad)


def check(got, want, grad_rtol=1e-5, grad_atol=1e-6):
    gl, gs, gdl, gdq, gdv = got
    wl, ws, wdl, wdq, wdv = want
    torch.testing.assert_close(gl, wl.float(), rtol=1e-5, atol=1e-6)
    for k in KEYS:
        torch.testing.assert_close(gs[k], ws[k].float(), rtol=1e-5, atol=1e-6, msg=k)
    torch.testing.assert_close(gdl.float(), wdl, rtol=grad_rtol, atol=grad_atol)
    for a, b in zip(gdq, wdq):
        torch.testing.assert_close(a.float(), b, rtol=grad_rtol, atol=grad_atol)
    torch.testing.assert_close(gdv.float(), wdv, rtol=1e-5, atol=1e-6)


def make_case(B, L, V, seed, dtype=torch.float32, prompt=1, ragged=True, nq=2, peaked=False):
    """Synthetic ILQL batch in the offline orchestrator's layout (offline_orchestrator.py:
    28-73): actions_ixs = arange(prompt-1, L-1), states one longer, dones 1 but the last."""
    g = torch.Generator().manual_seed(seed)
    A = L - prompt
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[0, -1] = V - 1
    ids[-1, 1] = 0
    attn = torch.ones(B, L, dtype=torch.long)
    dones = torch.ones(B, A + 1, dtype=torch.long)
    dones[:, -1] = 0
    if ragged and B > 1:  # padded rows (pad_sequence zeros) of different lengths
        for r in range(1, B, 2):
            cut = 1 + (r * 7) % (L - 1)
            attn[r, cut:] = 0
            dones[r, max(0, cut - prompt):] = 0
    aix = torch.arange(prompt - 1, L - 1).repeat(B, 1)
    six = torch.arange(prompt - 1, L).repeat(B, 1)
    rewards = torch.randn(B, A, generator=g)
    sc = 4.0 if peaked else 1.0
    logits = (torch.randn(B, L, V, generator=g) * sc).to(dtype)
    qs = [(torch.randn(B, A, V, generator=g) * sc).to(dtype) for _ in range(nq)]
    tqs = [(torch.randn(B, A, V, generator=g) * sc).to(dtype) for _ in range(nq)]
    vs = torch.randn(B, A + 1, 1, generator=g)
    return logits, qs, tqs, vs, P.ILQLBatch(ids, attn, rewards, six, aix, dones)


# ------------------------------------------------------------------ the fp64 reference and the bar
def oracle64(logits, qs, tqs, vs, batch, prec=torch.float64, **kw):
    """(loss, stats, dlogits, dq, dvs) of oracle.ppo_oracle.ilql_loss run in `prec` (fp64: the
    reference; fp32: the precondition of the CPU file) on the inputs as they are quantised."""
    def leaf(x):
        return x.detach().to(prec, copy=True).requires_grad_(True)

    lg, q, v = leaf(logits), [leaf(x) for x in qs], leaf(vs)
    loss, stats = orc.ilql_loss(lg, q, [x.to(prec) for x in tqs], v, batch.input_ids, batch.attention_mask,
                                batch.rewards.to(prec), batch.actions_ixs, batch.dones, **kw)
    loss.backward()
    B, S = batch.dones.shape
    return (loss.detach(), {k: stats[f"losses/{k}"].detach() for k in KEYS}, lg.grad, [x.grad for x in q],
            v.grad.reshape(B, S))


def bar(dtype):
    """The project's bar for the row gradients (the losses, stats and dvs are always fp32)."""
    return dict(rtol=1e-2, atol=2e-6) if dtype == torch.bfloat16 else dict(rtol=1e-5, atol=1e-6)


def check64(got, want, dtype=torch.float32, equal_nan=False):
    """got: (loss, stats | losses[5], dlogits, [dq], dvs) in any precision / device; want: oracle64."""
    gl, gs, gdl, gdq, gdv = got
    wl, ws, wdl, wdq, wdv = want
    if not isinstance(gs, dict):  # losses[5] in ilql._SLOT order
        gs = {k: gs[i] for i, k in enumerate(KEYS)}
    kw = dict(equal_nan=equal_nan)
    torch.testing.assert_close(gl.double().cpu().reshape(()), wl.double(), rtol=1e-5, atol=1e-6, msg="loss", **kw)
    for k in KEYS:
        torch.testing.assert_close(gs[k].double().cpu().reshape(()), ws[k].double(), rtol=1e-5, atol=1e-6,
                                   msg=lambda m, k=k: f"{k}: {m}", **kw)
    torch.testing.assert_close(gdl.double().cpu(), wdl.double(), msg=lambda m: f"dlogits: {m}", **bar(dtype), **kw)
    for i, (a, b) in enumerate(zip(gdq, wdq)):
        torch.testing.assert_close(a.double().cpu(), b.double(), msg=lambda m, i=i: f"dq{i}: {m}", **bar(dtype),
                                   **kw)
    torch.testing.assert_close(gdv.double().cpu().reshape(wdv.shape), wdv.double(), rtol=1e-5, atol=1e-6,
                               msg=lambda m: f"dvs: {m}", **kw)


# ------------------------------------------------------------------ the launch table, restated
NVS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16)           # kIlqlNVs
SPLITS = {0: (20, 5), 1: (22, 3), 2: (21, 4), 3: (19, 6)}  # ilql_split -> (NV, NL) of k_ilql_rows<F32T, NV, NL>
LINE_VECS, WAVE, MAX_THREADS = 16, 64, 1024
V_LAST = {F32: 65475, BF16: 130951}                        # the last V that fits; V_LAST + 1 -> TRLX_ERR_SHAPE


def esize(dtype):
    return 2 if dtype == torch.bfloat16 else 4


def vec_bound(V, dtype):
    """The host's bound on body vectors + line shift (ilql_geometry / ilql_launch_rows)."""
    return V // (16 // esize(dtype)) + 1 + (LINE_VECS - 1)


def select(dtype, V, split_lds=0, ilql_split=0):
    """(path, NV, NL, threads) that trlx_ilql_rows launches, or None where it returns
    TRLX_ERR_SHAPE.  path: "split" (VGPR + LDS residency, fp32 only) or "reg"."""
    n = vec_bound(V, dtype)
    if dtype == torch.float32 and split_lds != 1 and 512 * 16 < n <= 512 * 25:
        nv, nl = SPLITS[ilql_split]
        return "split", nv, nl, 512
    for pref in (512, MAX_THREADS):
        need = -(-n // pref)
        for c in NVS:
            if c >= need:
                thr = -(-(-(-n // c)) // WAVE) * WAVE
                return "reg", c, 0, max(thr, WAVE)
    return None


def entry_of(sel):
    """The instantiation and workgroup class of a selection: (path, NV, NL, 512 | 1024)."""
    return None if sel is None else (sel[0], sel[1], sel[2], 512 if sel[3] <= 512 else 1024)


# The V of the launch-table cases, per (dtype, split_lds).  Each line is one entry's smallest and
# largest V (tests/test_ilql_loss_table.py proves it against `select` over every V): which
# instantiation a case runs is known by reading.  fp32 rows hold 4 elements per vector, bf16 8;
# an entry of NV vectors x T threads holds V // EPV + 16 <= NV * T.
TABLE_V = {
    (F32, 0): [
        1, 2, 3, 4, 5,            # EPV-1, EPV, EPV+1 and below: head / tail only, one body vector
        1987,                     # NV 1   (1 .. 1987)
        1988, 4035,               # NV 2
        4036, 6083,               # NV 3
        6084, 8131,               # NV 4
        8132, 10179,              # NV 5
        10180, 12227,             # NV 6
        12228, 14275,             # NV 7
        14276, 16323,             # NV 8
        16324, 20419,             # NV 10  (need 9 and 10)
        20420, 24515,             # NV 12  (need 11 and 12)
        24516, 26563,             # NV 13
        26564, 32707,             # NV 16  (need 14, 15, 16); nvec bound 8192 |
        32708, 51139,             # split 20+5 (or 22+3 / 21+4 / 19+6): bound 8193 .. 12800 |
        51140, 53187,             # NV 13 x 1024: bound 12801 ..
        53188, 65475,             # NV 16 x 1024 .. the last V that fits
        50257,                    # the C5 vocabulary (split)
    ],
    (F32, 1): [                   # split_lds = 1: the same V without the split path
        32708, 40899,             # NV 10 x 1024
        40900, 49091,             # NV 12 x 1024
        49092, 51139, 50257,      # NV 13 x 1024 (51140 .. 53187 above)
    ],
    (BF16, 0): [
        1, 2, 3, 7, 8, 9,
        3975,                     # NV 1   (1 .. 3975)
        3976, 8071,               # NV 2
        8072, 12167,              # NV 3
        12168, 16263,             # NV 4
        16264, 20359,             # NV 5
        20360, 24455,             # NV 6
        24456, 28551,             # NV 7
        28552, 32647,             # NV 8
        32648, 40839,             # NV 10
        40840, 49031,             # NV 12
        49032, 53127,             # NV 13
        53128, 65415,             # NV 16; nvec bound 8192 | 8193
        65416, 81799,             # NV 10 x 1024
        81800, 98183,             # NV 12 x 1024
        98184, 106375,            # NV 13 x 1024
        106376, 130951,           # NV 16 x 1024 .. the last V that fits
    ],
}
# ilql_split 1..3 at the split range's two ends and at the C5 vocabulary
SPLIT_V = (32708, 50257, 51139)
# entries whose NV is larger than the row needs (need 9 -> NV 10, 11 -> 12, 14 / 15 -> 16): whole
# steps are out of range for some or all lanes.  (dtype, split_lds, V): the largest V of each need.
OVERSIZED_V = [(F32, 0, 18371), (F32, 0, 22467), (F32, 0, 28611), (F32, 0, 30659),
               (BF16, 0, 36743), (BF16, 0, 44935), (BF16, 0, 57223), (BF16, 0, 61319),
               (F32, 1, 36803), (F32, 1, 44995), (F32, 0, 57283), (F32, 0, 61379),
               (BF16, 0, 73607), (BF16, 0, 89991), (BF16, 0, 114567), (BF16, 0, 122759)]


def table_cases():
    """(dtype, V, split_lds, ilql_split) of every launch-table case of the GPU file, no repeats."""
    out = []
    for (dt, sl), vs in TABLE_V.items():
        out += [(dt, v, sl, 0) for v in vs]
    out += [(dt, v, sl, 0) for dt, sl, v in OVERSIZED_V]
    out += [(F32, v, 0, k) for k in (1, 2, 3) for v in SPLIT_V]
    return list(dict.fromkeys(out))


# ------------------------------------------------------------------ the row geometry, restated
def row_split(ptr, V, es):
    """(head, nvec, tail0, tail, shift) of a row at byte address ptr: common.h RowSplit and
    line_shift(row + head)."""
    epv = 16 // es
    head = min(((16 - (ptr & 15)) & 15) // es, V)
    nvec = (V - head) // epv
    tail0 = head + nvec * epv
    return head, nvec, tail0, V - tail0, ((ptr + head * es) >> 4) & 15


def locate(ptr, V, dtype, sel, j):
    """Where k_ilql_rows holds element j of the row at ptr: ("head", j) / ("tail", j - tail0), or
    ("vgpr" | "lds", step, lane, vector, element of the vector)."""
    es = esize(dtype)
    epv = 16 // es
    head, nvec, tail0, tail, shift = row_split(ptr, V, es)
    assert 0 <= j < V
    if j < head:
        return ("head", j)
    if j >= tail0:
        return ("tail", j - tail0)
    _, nv, nl, thr = sel
    i = (j - head) // epv
    step, lane = divmod(i + shift, thr)
    assert step < nv + nl, "the row does not fit its instantiation"
    return ("vgpr" if step < nv else "lds", step, lane, i, (j - head) % epv)


def y_positions(ptr, V, dtype, sel):
    """{name: token} placing the action token at every store site of gy for the row at ptr: each
    head and tail element, the first and last element of body vector 0, the last body vector, a
    vector of step 0 and of the last VGPR step that holds one, and for the split kernel a vector
    of the first and of the last LDS step."""
    es = esize(dtype)
    epv = 16 // es
    head, nvec, tail0, tail, shift = row_split(ptr, V, es)
    _, nv, nl, thr = sel
    pos = {f"head{e}": e for e in range(head)}
    pos.update({f"tail{e}": tail0 + e for e in range(tail)})
    if nvec:
        last_step = (nvec - 1 + shift) // thr

        def in_step(k, lane_off):  # a vector of step k, lane_off lanes into it (clipped to the body)
            i = min(max(k * thr - shift, 0) + lane_off, nvec - 1)
            return head + i * epv + (i % epv)

        pos.update({"vec0_first": head, "vec0_last": head + epv - 1,
                    "last_vec": head + (nvec - 1) * epv + epv // 2,
                    "step0": in_step(0, 1), "vgpr_last_step": in_step(min(nv - 1, last_step), 3)})
        if nl:
            pos.update({"lds_first_step": in_step(nv, 7), "lds_last_step": in_step(min(nv + nl - 1, last_step), 70)})
    return pos


# ------------------------------------------------------------------ placed rows and the direct ABI
def phased(block, p0, sb_bytes, st_bytes, fill=FILL):
    """Copy a [B, T, V] CPU tensor into a wider device buffer of `fill`: row (0, 0) starts p0 bytes
    past a 256-B boundary, row (b, t) a further b * sb_bytes + t * st_bytes (mod 256); at least
    one element of fill lies between any two rows.  Returns the strided [B, T, V] view."""
    B, T, V = block.shape
    es = block.element_size()
    per = 256 // es

    def stride(at_least, phase_bytes):  # smallest count >= at_least with count * es = phase_bytes (mod 256)
        assert phase_bytes % es == 0
        return at_least + (phase_bytes // es - at_least) % per

    st = stride(V + 1, st_bytes)
    sb = stride(T * st + 1, sb_bytes)
    buf = torch.full((3 * per + (B - 1) * sb + (T - 1) * st + V,), fill, dtype=block.dtype, device=DEV)
    off = per + ((p0 - buf.data_ptr() - per * es) % 256) // es
    view = buf.as_strided((B, T, V), (sb, st, 1), off)
    view.copy_(block)
    assert view.data_ptr() % 256 == p0
    return view


def row_ptrs(view):
    """Byte address of every row (b, t) of a [B, T, V] view, as a [B][T] list."""
    es = view.element_size()
    B, T, _ = view.shape
    return [[view.data_ptr() + (b * view.stride(0) + t * view.stride(1)) * es for t in range(T)] for b in range(B)]


def covered(view):
    """Bool mask over view's backing buffer: the elements that belong to a row of the view."""
    base = view._base if view._base is not None else view
    m = torch.zeros(base.numel(), dtype=torch.bool, device=base.device)
    m.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    return base.reshape(-1), m


def filled_grad(x, fill=FILL):
    """grad_buffer_like(x) (the rows' 256-B phase) with the whole backing buffer set to fill."""
    g = grad_buffer_like(x)
    (g._base if g._base is not None else g).fill_(fill)
    return g


class Out:
    """What one direct call left: rc, message, losses[5], dlogits, dq, dvs (device tensors)."""


def launch(lg, qs, tqs, vs, rewards, ids, attn, aix, dones, hp=None, gathered=False, dlg=None, dqs=None,
           fn="trlx_ilql_loss_fused", workspace=None):
    """One trlx_ilql_* call on device tensors as they are (row strides from the tensors; tqs fp32
    [B, A] when gathered).  Gradient rows, dvs and losses are FILL before the call.  No raise: the
    status is returned in Out.rc."""
    hp = dict(dict(tau=0.7, gamma=0.99, cql_scale=0.1, awac_scale=1.0), **(hp or {}))
    B, L, V = lg.shape
    A, nq = qs[0].shape[1], len(qs)
    o = Out()
    o.dlogits = filled_grad(lg) if dlg is None else dlg
    o.dq = [filled_grad(q) for q in qs] if dqs is None else dqs
    o.dvs = torch.full((B, A + 1), FILL, dtype=torch.float32, device=DEV)
    o.losses = torch.full((5,), FILL, dtype=torch.float32, device=DEV)
    o.workspace = workspace if workspace is not None else torch.zeros(
        _lib.query("trlx_ilql_workspace_bytes", B, L, A, nq), dtype=torch.uint8, device=DEV)
    a = _lib.IlqlArgs()
    a.dtype, a.nq, a.B, a.L, a.A, a.V = _lib.dtype_code(lg), nq, B, L, A, V
    a.tq_gathered = int(gathered)
    a.logits, a.logits_sb, a.logits_st = lg.data_ptr(), lg.stride(0), lg.stride(1)
    a.dlogits, a.dlogits_sb, a.dlogits_st = o.dlogits.data_ptr(), o.dlogits.stride(0), o.dlogits.stride(1)
    for i in range(nq):
        a.q[i], a.tq[i], a.dq[i] = qs[i].data_ptr(), tqs[i].data_ptr(), o.dq[i].data_ptr()
        a.q_sb[i], a.q_st[i] = qs[i].stride(0), qs[i].stride(1)
        a.tq_sb[i], a.tq_st[i] = tqs[i].stride(0), tqs[i].stride(1)
        a.dq_sb[i], a.dq_st[i] = o.dq[i].stride(0), o.dq[i].stride(1)
    for name, t in (("input_ids", ids), ("attention_mask", attn), ("actions_ixs", aix), ("dones", dones)):
        assert t.dtype == torch.int64 and t.is_contiguous() and t.is_cuda
        setattr(a, name, t.data_ptr())
    assert vs.is_contiguous() and rewards.is_contiguous() and vs.numel() == B * (A + 1)
    a.rewards, a.rewards_dtype = rewards.data_ptr(), _lib.dtype_code(rewards)
    a.vs, a.vs_dtype = vs.data_ptr(), _lib.dtype_code(vs)
    a.tau, a.gamma, a.cql_scale, a.awac_scale = hp["tau"], hp["gamma"], hp["cql_scale"], hp["awac_scale"]
    a.dvs, a.losses, a.workspace = o.dvs.data_ptr(), o.losses.data_ptr(), o.workspace.data_ptr()
    lib = _lib.load()
    o.rc = getattr(lib, fn)(ctypes.byref(a), _lib.stream_of(lg))
    o.msg = lib.trlx_last_error().decode(errors="replace") if o.rc else ""
    torch.cuda.synchronize()
    return o


def launch_case(case, at=None, vs_dtype=None, rewards_dtype=None, gathered_tq=None, **kw):
    """launch() from a Case's CPU tensors.  at: {"logits" | "q0" | "q1": (p0, sb_bytes, st_bytes)}
    places that tensor with phased(); the others are contiguous copies.  Returns (Out, views)."""
    at = at or {}

    def stage(t, key):
        return phased(t, *at[key]) if key in at else t.to(DEV).contiguous()

    views = {"logits": stage(case.logits, "logits")}
    for i, q in enumerate(case.qs):
        views[f"q{i}"] = stage(q, f"q{i}")
    b = case.batch
    tqs = [t.to(DEV).contiguous() for t in (case.tqs if gathered_tq is None else gathered_tq)]
    o = launch(views["logits"], [views[f"q{i}"] for i in range(len(case.qs))], tqs,
               case.vs.to(DEV, vs_dtype or torch.float32).contiguous(),
               b.rewards.to(DEV, rewards_dtype or torch.float32).contiguous(), b.input_ids.to(DEV),
               b.attention_mask.to(DEV), b.actions_ixs.to(DEV), b.dones.to(DEV), hp=case.hp,
               gathered=gathered_tq is not None, **kw)
    return o, views


def got_of(o):
    return o.losses[0], o.losses, o.dlogits, o.dq, o.dvs


def gaps_untouched(o):
    """Every element of the gradient buffers outside the rows still holds FILL."""
    for g in [o.dlogits] + o.dq:
        base, m = covered(g)
        rest = base[~m]
        if not bool((rest == FILL).all()):
            return False
    return True


# ------------------------------------------------------------------ the input sets
class Case:
    """CPU inputs of one launch and the loss's hyper-parameters (hp: oracle keyword arguments)."""

    def __init__(self, logits, qs, tqs, vs, batch, hp=None, dtype=None):
        self.logits, self.qs, self.tqs, self.vs, self.batch = logits, qs, tqs, vs, batch
        self.hp = hp or {}
        self.dtype = dtype or logits.dtype

    @property
    def nq(self):
        return len(self.qs)

    def clone(self):
        b = P.ILQLBatch(*(getattr(self.batch, f).clone() for f in FIELDS))
        return Case(self.logits.clone(), [q.clone() for q in self.qs], [q.clone() for q in self.tqs],
                    self.vs.clone(), b, dict(self.hp), self.dtype)

    def want(self, prec=torch.float64):
        return oracle64(self.logits, self.qs, self.tqs, self.vs, self.batch, prec=prec, **self.hp)


def rows_case(B, L, V, seed, dtype=torch.float32, prompt=1, nq=2, ragged=False, offset=-20.0, peaks=True, hp=None):
    """make_case with the rows moved to where a wrong lane predicate shows.  Every row is shifted
    by `offset` (-20): an out-of-range lane loads 0, which then is the row's maximum by far and
    e^20 of its Σexp, where among N(0, 1) logits it would hide below the bar.  peaks: each row
    gets +10 at one element of a fixed edge list (last, first, one vector in from either end,
    the middle), so a vector dropped from the sum moves the row's lse by O(1); every second group
    of six rows gets +120 instead, so a vector dropped from the maximum overflows exp (the lse does
    not depend on the offset m subtracted inside exp until then)."""
    logits, qs, tqs, vs, b = make_case(B, L, V, seed, dtype=torch.float32, prompt=prompt, ragged=ragged, nq=nq)
    epv = 16 // esize(dtype)
    edge = [V - 1, 0, max(V - 1 - epv, 0), min(epv, V - 1), V // 2, max(V - 1 - 2 * epv, 0)]
    r = 0
    for t in [logits] + qs:
        t += offset
        if peaks:
            flat = t.view(-1, V)
            for i in range(flat.shape[0]):
                flat[i, edge[r % len(edge)]] += 120.0 if (r // len(edge)) % 2 else 10.0
                r += 1
    return Case(logits.to(dtype), [q.to(dtype) for q in qs], [q.to(dtype) for q in tqs], vs, b, hp, dtype)


def table_nq(V, split_lds=0, ilql_split=0):
    """Two Q heads, but one in a few default-knob cases (V = 3 mod 8: most fp32 entries' largest V)."""
    return 1 if V % 8 == 3 and V > 8 and not split_lds and not ilql_split else 2


@functools.lru_cache(maxsize=None)
def table_case(dtype, V, prompt, nq=2):
    return rows_case(2, 4, V, 1000 + V + prompt, dtype=dtype, prompt=prompt, nq=nq)


# Phased rows: (B, L, p0, sb_bytes, st_bytes) per dtype such that the B x (L - 1) rows that carry a
# loss (and the B x A Q rows, A = L - 1) cover every line shift 0..15 and every head length
# 0..EPV-1 (asserted on the host from data_ptr() and the strides).  fp32: b moves the row 20 B
# (one shift, one head element less), t 64 B (4 shifts); bf16: b 18 B, t 128 B (8 shifts).
PHASE_LAYOUT = {F32: (4, 5, 4, 20, 64), BF16: (8, 3, 2, 18, 128)}
# small | 1024 threads (bf16 has no split path) or split | the largest split V | the largest V
PHASE_V = {F32: (1031, 40001, 51139, 65475), BF16: (1031, 100003, 130951)}


@functools.lru_cache(maxsize=None)
def phase_case(dtype, V):
    B, L = PHASE_LAYOUT[dtype][:2]
    return rows_case(B, L, V, 2000 + V, dtype=dtype, ragged=False)


def phase_cover(view, rows_t):
    """(set of line shifts, set of head lengths) over rows (b, t < rows_t) of a view."""
    es = view.element_size()
    V = view.shape[-1]
    geo = [row_split(p, V, es) for r in row_ptrs(view) for p in r[:rows_t]]
    return {g[4] for g in geo}, {g[0] for g in geo}


# Position of the action token: one register-resident and one split-path (bf16: 1024-thread) V
# per dtype whose rows, placed one element before a 16-B boundary... p0 = 16 * 5 + es puts every
# row at head EPV-1 and line shift 6; V = EPV-2 (mod EPV) then leaves EPV-1 tail elements.
YPOS_V = {F32: (10002, 51134), BF16: (20006, 100006)}


def ypos_p0(dtype):
    return 16 * 5 + esize(dtype)


def ypos_case(dtype, V, ilql_split=0):
    """B = 1; logits row t and Q rows a = t share one 256-B phase, so one token list places y at
    position k of y_positions in logits row k and in the Q rows of action k."""
    pos = y_positions(ypos_p0(dtype), V, dtype, select(dtype, V, 0, ilql_split))
    n = len(pos)
    c = rows_case(1, n + 1, V, 3000 + V, dtype=dtype, ragged=False, peaks=False, offset=0.0)
    c.batch.input_ids[0, 1:] = torch.tensor(list(pos.values()))
    return c, pos


def perm_case(kind):
    """actions_ixs permuted / with repeats / two actions at one token (B 3, L 8, prompt 2, V 37)."""
    c = rows_case(3, 8, 37, 4000, prompt=2, ragged=True, offset=0.0, peaks=False)
    A, L = 6, 8
    g = torch.Generator().manual_seed(41)
    if kind == "perm":
        aix = torch.stack([torch.randperm(L - 1, generator=g)[:A] for _ in range(3)])
    elif kind == "repeat":
        aix = torch.randint(0, L - 1, (3, A), generator=g)
        aix[0, 1] = aix[0, 0]
    else:  # every action of a row at one token
        aix = torch.tensor([[0] * A, [L - 2] * A, [3] * A])
    c.batch.actions_ixs = aix
    return c


# Reductions: (B, L, prompt, V, nq).  Prep sums B * A dones and B * (L - 1) attention elements in
# blocks of 256, at most 128 blocks (> 32768 elements: chunks longer than 256); finalize sums the
# row records in blocks of 1024, at most 128 (> 131072 rows).
RED_SHAPES = {
    "prep_multi_p3": (20, 20, 3, 5, 2),            # 380 attention / 340 dones elements: 2 blocks, A != L-1
    "prep_multi_pL2": (20, 20, 18, 5, 2),          # A = 2: the dones space ends inside block 0
    "prep_32768": (1024, 33, 3, 3, 2),             # exactly 128 blocks of 256
    "prep_32800": (1025, 33, 3, 3, 1),             # 129 -> 128 blocks of 257
    "prep_32800_pL2": (1025, 33, 31, 3, 2),
    "fin_147150": (450, 111, 3, 3, 2),             # 147150 rows > 131072: finalize chunks of 1150
    "hot_148950": (450, 111, 1, 3, 2),             # A = L-1 (ILQLHotPath): both caps
}
# the CPU precondition's slice of the > 100k-row cases
RED_SLICE = {"fin_147150": (16, 111, 3, 3, 2), "hot_148950": (16, 111, 1, 3, 2)}


@functools.lru_cache(maxsize=None)
def red_case(name, variant="ragged", sliced=False):
    """variant: ragged (padded rows of different lengths) | ones (no zero weight: the fast path) |
    done_zero (a single zero at dones[B-1, A-1]) | attn_zero (attention_mask[B-1, L-1]) |
    no_dones (every done 0: n = max(1, 0), every Q row skipped)."""
    B, L, prompt, V, nq = (RED_SLICE if sliced else RED_SHAPES)[name]
    c = rows_case(B, L, V, 5000 + B + L + prompt, prompt=prompt, nq=nq, ragged=variant == "ragged", offset=0.0,
                  peaks=False)
    A = L - prompt
    if variant == "done_zero":
        c.batch.dones[B - 1, A - 1] = 0
    elif variant == "attn_zero":
        c.batch.attention_mask[B - 1, L - 1] = 0
    elif variant == "no_dones":
        c.batch.dones[:] = 0
    return c


def scalar_case(kind="plain", nq=2, dtype=torch.float32):
    """B 3, L 7, prompt 2, V 1031 with ragged rows; kind: plain | tie (vs[2, 2] made exactly the
    minimum target Q at its action) | tq_nan (target head 1 NaN at the action of (2, 2))."""
    c = rows_case(3, 7, 1031, 6000 + nq, dtype=dtype, prompt=2, nq=nq, ragged=True, offset=0.0, peaks=False)
    b = c.batch
    y = int(b.input_ids[2, 1 + int(b.actions_ixs[2, 2])])
    assert int(b.dones[2, 2]) == 1
    if kind == "tie":
        c.vs[2, 2, 0] = min(float(t[2, 2, y]) for t in c.tqs)
    elif kind == "tq_nan":
        c.tqs[-1][2, 2, y] = float("nan")
    return c


def mask_first_case():
    """B 3, L 6, prompt 2, V 37: sequence 1 is padding from token 1 on (every logits row of it, row 0
    included, and every Q row has zero weight); sequence 2 ends one token early."""
    c = rows_case(3, 6, 37, 7000, prompt=2, offset=0.0, peaks=False)
    c.batch.attention_mask[1, 1:] = 0
    c.batch.dones[1, :] = 0
    c.batch.attention_mask[2, -1] = 0
    c.batch.dones[2, -2:] = 0
    return c


def cpu_cases():
    """name -> builder of every input set whose precondition the CPU file checks."""
    out = {}
    for dt, V, sl, k in table_cases():
        if k == 0:
            for prompt in (1, 2):
                out[f"table-{esize(dt) * 8}-{V}-p{prompt}"] = functools.partial(table_case, dt, V, prompt,
                                                                                table_nq(V, sl, k))
    for dt in (F32, BF16):
        for V in PHASE_V[dt]:
            out[f"phase-{esize(dt) * 8}-{V}"] = functools.partial(phase_case, dt, V)
        for V in YPOS_V[dt]:  # (the token list of ilql_split 1..3 moves two tokens; the rows are the same)
            out[f"ypos-{esize(dt) * 8}-{V}"] = lambda dt=dt, V=V: ypos_case(dt, V)[0]
    for kind in ("perm", "repeat", "same"):
        out[f"aix-{kind}"] = functools.partial(perm_case, kind)
    for name in RED_SHAPES:
        for variant in ("ragged", "ones", "done_zero", "attn_zero", "no_dones"):
            out[f"red-{name}-{variant}"] = functools.partial(red_case, name, variant, name in RED_SLICE)
    out["mask-first"] = mask_first_case
    for kind in ("plain", "tie"):
        for nq in (1, 2):
            out[f"scalar-{kind}-nq{nq}"] = functools.partial(scalar_case, kind, nq)
    for tau in (0.0, 1.0):
        def with_tau(tau=tau):
            c = scalar_case("plain")
            c.hp = dict(tau=tau)
            return c
        out[f"scalar-tau{tau}"] = with_tau
    return out
