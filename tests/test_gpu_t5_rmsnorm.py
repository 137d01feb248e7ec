"""The T5 RMSNorm with residual add on the device: trlx_t5_rmsnorm_fwd / _bwd, t5_rmsnorm,
t5_add_rmsnorm and T5LayerNorm.

Parity is per element under the rule of t5_rmsnorm_checks (|got - ref| <= ulp(|ref|) + 2^-16 M against
the float64 oracle), for both dtypes and every combination of optional operand, at sizes taken from
trlx_t5_rmsnorm_geometry at collection time: every kernel form's largest D and the first D of the
next, N around the rows of a workgroup pass, an N that gives exactly G partials and one past it, where
a workgroup walks two row blocks.  What no tolerance can hide is checked in bits: the add against
torch's, the add form against the norm of the sum, the two access forms, layouts, in place, saved
against recomputed rstd, run to run, sentinels, refusals.  TRLX_T5_RMSNORM_PARITY_OUT=<file> writes
the measured figures: per dtype and output the kernel's worst ratio to the rule and HF's eager op
sequence's."""
import ctypes
import json
import os

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_rmsnorm_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 77.0
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
GEO = P.t5_norm.geometry()
WORST = {}       # (route, dtype name, output) -> worst ratio
MEMORY = {}


def vec_of(dtype):
    return GEO["vec_bf16"] if dtype == torch.bfloat16 else GEO["vec_f32"]


def widths(dtype):
    """D: 1, 7, one vector, one more, the model widths, and both sides of every form's limit."""
    v = vec_of(dtype)
    ds = {1, 7, v, v + 1, 96, 512, 768, 1024, 4096, GEO["reg_max_d"], GEO["max_d"]}
    for b in GEO["d_breaks"]:
        ds |= {b, b + v, b + 1}
    return sorted(d for d in ds if d <= GEO["max_d"])


def heights(D):
    rpb = P.t5_norm.geometry(1, D)["rows_per_block"]
    return sorted({1, max(rpb - 1, 1), rpb + 1})


def walk_heights(D):
    """N with exactly G = max_partials partial rows, and the first N at which a workgroup walks two blocks."""
    rpb = P.t5_norm.geometry(1, D)["rows_per_block"]
    return [rpb * GEO["max_partials"], rpb * GEO["max_partials"] + 1]


@pytest.fixture(scope="module", autouse=True)
def figures_file():
    yield
    path = os.environ.get("TRLX_T5_RMSNORM_PARITY_OUT")
    if path and WORST:
        rec = {"rule": "|got - ref| <= ulp_dtype(|ref|) + 2^-16 * M per element against the float64 oracle; figures are "
                       "the worst ratio to that bound over every case, combination of operands and element",
               "geometry": {k: (list(v) if isinstance(v, tuple) else v) for k, v in GEO.items()}, "worst_ratio": {},
               "memory": MEMORY}
        for (route, dt, out), r in sorted(WORST.items()):
            rec["worst_ratio"].setdefault(route, {}).setdefault(dt, {})[out] = r
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)


def note(route, dtype, figs):
    name = {v: k for k, v in DTYPES.items()}[dtype]
    for out, r in figs.items():
        WORST[(route, name, out)] = max(WORST.get((route, name, out), 0.0), r)


# ------------------------------------------------------------------ the C ABI on 2-D views
def code(dtype):
    return _lib.BF16 if dtype == torch.bfloat16 else _lib.F32


def raw_args(N, D, dtype, eps=C.EPS, w=None, dw=None, rstd=None, ws=None, **rows):
    kw = {}
    for name in ("x", "residual", "h", "y", "dy", "dh_in", "dh"):
        t = rows.get(name)
        kw[name] = None if t is None else t.data_ptr()
        kw[f"ld_{name}"] = D if t is None else (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), D))
    return _lib.T5RmsNormArgs(N=N, D=D, eps=eps, dtype=code(dtype), w=_lib.ptr(w), dw=_lib.ptr(dw), rstd=_lib.ptr(rstd),
                              ws=_lib.ptr(ws), ws_bytes=0 if ws is None else ws.numel() * 4, **kw)


def call(entry, *a, **k):
    _lib.call(entry, ctypes.byref(raw_args(*a, **k)), torch.cuda.current_stream(DEV).cuda_stream)


def fwd(x, w, residual=None, rstd=True, h_out=None, eps=C.EPS):
    N, D = x.shape
    y = torch.full((N, D), SENTINEL, dtype=x.dtype, device=DEV)
    h = None
    if residual is not None:
        h = torch.full((N, D), SENTINEL, dtype=x.dtype, device=DEV) if h_out is None else h_out
    r = torch.full((N,), SENTINEL, dtype=torch.float32, device=DEV) if rstd else None
    call("trlx_t5_rmsnorm_fwd", N, D, x.dtype, eps, w=w, rstd=r, x=x, residual=residual, h=h, y=y)
    return h, y, r


def bwd(h, w, dy, dh_in=None, rstd=None, want_dh=True, want_dw=True, eps=C.EPS):
    N, D = h.shape
    dh = torch.full((N, D), SENTINEL, dtype=h.dtype, device=DEV) if want_dh else None
    dw = torch.full((D,), SENTINEL, dtype=h.dtype, device=DEV) if want_dw else None
    ws = None
    if want_dw:
        q = P.t5_norm.geometry(N, D)
        ws = torch.full((q["ws_bytes"] // 4 + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    call("trlx_t5_rmsnorm_bwd", N, D, h.dtype, eps, w=w, dw=dw, rstd=rstd, ws=ws, h=h, dy=dy, dh_in=dh_in, dh=dh)
    if ws is not None:
        assert bool((ws[-64:] == SENTINEL).all()), "the workspace was written past G * D"
    return dh, dw


def on_device(c):
    return {k: t.to(DEV) for k, t in c.items()}


def full_check(N, D, dtype):
    """Forward in both forms and the backward in every combination of dh_in, rstd, dh, dw."""
    c = C.case(N, D, dtype)
    d = on_device(c)
    hsum = C.rounded_sum(c)
    M = {True: C.factors(hsum, c["w"], c["dy"], c["dh_in"]), False: C.factors(hsum, c["w"], c["dy"])}
    want = {True: C.oracle(hsum, c["w"], c["dy"], c["dh_in"]), False: C.oracle(hsum, c["w"], c["dy"])}
    h, y, rstd = fwd(d["x"], d["w"], d["residual"])
    assert torch.equal(h, d["residual"] + d["x"]) and torch.equal(h.cpu(), hsum)       # bit for bit torch's add
    h1, y1, rstd1 = fwd(h, d["w"])                                                     # the norm alone, of that sum
    assert h1 is None and torch.equal(y1, y) and torch.equal(rstd1, rstd)
    figs = C.judge({"y": y}, want[False], M[False], dtype)
    rr = float(((rstd.double().cpu() - want[False]["rstd"]).abs() / want[False]["rstd"]).max())
    assert rr <= 2.0 ** -20, (N, D, rr)
    first = {}
    for with_in in (True, False):
        for with_rstd in (True, False):
            for want_dh, want_dw in ((True, True), (True, False), (False, True)):
                if with_in and not want_dh:
                    continue
                dh, dw = bwd(h, d["w"], d["dy"], d["dh_in"] if with_in else None, rstd if with_rstd else None, want_dh, want_dw)
                got = {"dh": dh, "dw": dw}
                f = C.judge(got, want[with_in], M[with_in], dtype)
                for n, t in got.items():                      # every combination gives the same bits of what it shares
                    if t is not None:
                        key = (n, with_in if n == "dh" else None)
                        assert torch.equal(first.setdefault(key, t), t), (n, with_in, with_rstd, want_dh, want_dw)
                figs = {n: max(figs.get(n, 0.0), r) for n, r in {**figs, **f}.items()}
    torch.cuda.synchronize()
    print(N, D, dtype, figs)
    for n, r in figs.items():
        assert r <= 1.0, (N, D, dtype, n, figs)
    note("kernel", dtype, figs)
    if dtype == torch.bfloat16 and N > 1:
        note("hf_eager", dtype, C.judge(C.eager(h, d["w"], d["dy"], d["dh_in"]), want[True], M[True], dtype))


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
def test_parity_at_every_width_and_height(dtype):
    for D in widths(dtype):
        for N in heights(D):
            full_check(N, D, dtype)


@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("D", [96, GEO["wave_row_max_d"] + 8])
def test_parity_at_g_partials_and_where_a_workgroup_walks(D, dtype):
    for N in walk_heights(D):
        q = P.t5_norm.geometry(N, D)
        assert q["partials"] == GEO["max_partials"] and (q["row_blocks"] > q["partials"]) == (N != walk_heights(D)[0])
        full_check(N, D, dtype)


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("D", [64, 768, 1032, 4096])
def test_layouts_and_access_forms_give_the_same_bits(D, dtype):
    """The vector form on aligned contiguous rows against the element form (every operand one element
    off the 16-byte grid, odd row strides) and against strided rows that stay on the grid (a padded
    ld, the last step of a [B, T, D] tensor)."""
    N, v = 9, vec_of(dtype)
    d = on_device(C.case(N, D, dtype))
    h0, y0, r0 = fwd(d["x"], d["w"], d["residual"])
    dh0, dw0 = bwd(h0, d["w"], d["dy"], d["dh_in"], r0)

    def placed(t, ld, off):
        buf = torch.full((N * ld + off + 8,), SENTINEL, dtype=dtype, device=DEV)
        view = buf[off:off + N * ld].view(N, ld)[:, :D]
        view.copy_(t)
        return buf, view

    def blank(ld, off):
        buf = torch.full((N * ld + off + 8,), SENTINEL, dtype=dtype, device=DEV)
        return buf, buf[off:off + N * ld].view(N, ld)[:, :D]

    def untouched(buf, view):
        keep = torch.ones_like(buf, dtype=torch.bool)
        off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
        keep[off:off + N * view.stride(0)].view(N, -1)[:, :D] = False
        return bool((buf[keep] == SENTINEL).all())

    for ld, off in ((D + 3, 1), (D + v, 0), (D, 1)):
        ins = {k: placed(d[k], ld, off)[1] for k in ("x", "residual", "dy", "dh_in")}
        wbuf = torch.full((D + 8 + off,), SENTINEL, dtype=dtype, device=DEV)
        w = wbuf[off:off + D]
        w.copy_(d["w"])
        outs = {k: blank(ld, off) for k in ("h", "y", "dh")}
        dwbuf = torch.full((D + 8 + off,), SENTINEL, dtype=dtype, device=DEV)
        rstd = torch.empty(N, dtype=torch.float32, device=DEV)
        ws = torch.empty(P.t5_norm.geometry(N, D)["ws_bytes"] // 4, dtype=torch.float32, device=DEV)
        call("trlx_t5_rmsnorm_fwd", N, D, dtype, w=w, rstd=rstd, x=ins["x"], residual=ins["residual"], h=outs["h"][1], y=outs["y"][1])
        call("trlx_t5_rmsnorm_bwd", N, D, dtype, w=w, dw=dwbuf[off:off + D], rstd=rstd, ws=ws, h=outs["h"][1], dy=ins["dy"],
             dh_in=ins["dh_in"], dh=outs["dh"][1])
        for k, ref in (("h", h0), ("y", y0), ("dh", dh0)):
            assert torch.equal(outs[k][1], ref), (k, ld, off)
            assert untouched(*outs[k]), (k, ld, off)
        assert torch.equal(rstd, r0) and torch.equal(dwbuf[off:off + D], dw0)
        assert bool((dwbuf[:off] == SENTINEL).all()) and bool((dwbuf[off + D:] == SENTINEL).all())
    B, T = 3, 4                                                   # the last step of [B, T, D], and a [B, 1, D] slice
    big = torch.randn(B, T, D, device=DEV).to(dtype)
    wN = d["w"]
    for view in (big[:, -1, :], big[:, 1:2, :]):
        got = P.t5_rmsnorm(view, wN)
        assert torch.equal(got, P.t5_rmsnorm(view.contiguous(), wN)) and got.shape == view.shape
        assert P.t5_norm._rows(view, D).data_ptr() == view.data_ptr()       # read in place, no copy


@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
def test_in_place_add_and_two_runs(dtype):
    N, D = 11, 768
    d = on_device(C.case(N, D, dtype))
    h0, y0, r0 = fwd(d["x"], d["w"], d["residual"])
    for name in ("residual", "x"):                              # h written over residual, or over x
        ops = {k: d[k].clone() for k in ("x", "residual")}
        h, y, r = fwd(ops["x"], d["w"], ops["residual"], h_out=ops[name])
        assert h.data_ptr() == ops[name].data_ptr() and torch.equal(h, h0) and torch.equal(y, y0) and torch.equal(r, r0)
    xs = d["x"].clone()                                         # the norm alone over its own input
    call("trlx_t5_rmsnorm_fwd", N, D, dtype, w=d["w"], x=xs, y=xs)
    assert torch.equal(xs, fwd(d["x"], d["w"])[1])
    a, b = bwd(h0, d["w"], d["dy"], d["dh_in"], r0), bwd(h0, d["w"], d["dy"], d["dh_in"], r0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    dh_in = d["dh_in"].clone()                                  # dh over dh_in
    call("trlx_t5_rmsnorm_bwd", N, D, dtype, w=d["w"], rstd=r0, h=h0, dy=d["dy"], dh_in=dh_in, dh=dh_in)
    assert torch.equal(dh_in, a[0])


# ------------------------------------------------------------------ edge rows
def test_zero_overflow_and_nan_rows():
    D = 768
    c = C.case(6, D, torch.float32)
    h = C.rounded_sum(c)
    h[2] = 0.0
    h[3] = 3e19 * torch.sign(h[3] + 0.1)                         # the sum of squares overflows fp32
    clean = h.clone()
    h[4, 5] = float("nan")
    d = on_device(c)
    for dtype in (torch.float32, torch.bfloat16):
        hd, hc, w, dy = h.to(DEV).to(dtype), clean.to(DEV).to(dtype), d["w"].to(dtype), d["dy"].to(dtype)
        _, y, rstd = fwd(hd, w)
        _, yc, rstdc = fwd(hc, w)
        dh, dw = bwd(hd, w, dy, None, rstd)
        dhc, dwc = bwd(hc, w, dy, None, rstdc)
        assert bool((y[2] == 0).all()) and float(rstd[2]) == pytest.approx(C.EPS ** -0.5, rel=1e-6)
        assert bool(torch.isfinite(dh[2]).all()) and bool(torch.isfinite(dhc).all()) and bool(torch.isfinite(dwc).all())
        hf = C.hf_norm(hd.float(), w.float())                    # HF's fp32 expression: variance inf, y = 0, no NaN
        assert bool((hf[3] == 0).all()) and bool((y[3] == 0).all()) and float(rstd[3]) == 0.0
        assert bool(torch.isnan(y[4]).all()) and bool(torch.isnan(dh[4]).all()) and bool(torch.isnan(dw).all())
        rows = [0, 1, 2, 3, 5]                                   # a NaN changes no other row
        assert torch.equal(y[rows], yc[rows]) and torch.equal(dh[rows], dhc[rows])
        assert not bool(torch.isnan(y[rows]).any()) and not bool(torch.isnan(dh[rows]).any())


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize("dtype", list(DTYPES.values()), ids=list(DTYPES))
def test_autograd_through_the_add_form(dtype):
    B, T, D = 3, 7, 768
    c = C.case(B * T, D, dtype)
    d = on_device(c)
    x, r, w = (d[k].clone().requires_grad_() for k in ("x", "residual", "w"))
    m = P.T5LayerNorm(D).to(DEV).to(dtype)
    with torch.no_grad():
        m.weight.copy_(d["w"])
    h, y = m.add_forward(x.view(B, T, D), r.view(B, T, D))
    assert h.shape == y.shape == (B, T, D)
    gx, gr, gw = torch.autograd.grad([h, y], [x, r, m.weight], [d["dh_in"].view(B, T, D), d["dy"].view(B, T, D)])
    assert torch.equal(gx, gr)
    hsum = C.rounded_sum(c)
    want = C.oracle(hsum, c["w"], c["dy"], c["dh_in"])
    figs = C.judge({"y": y.detach().view(-1, D), "dh": gx, "dw": gw}, want, C.factors(hsum, c["w"], c["dy"], c["dh_in"]), dtype)
    assert max(figs.values()) <= 1.0, figs
    # only y used downstream, only h used downstream
    h2, y2 = P.t5_add_rmsnorm(x, r, w)
    (g1,) = torch.autograd.grad(y2, x, d["dy"], retain_graph=True)
    assert torch.equal(g1, bwd(h2.detach(), d["w"], d["dy"], None, None, True, False)[0])
    (g2,) = torch.autograd.grad(h2, r, d["dh_in"])
    assert torch.equal(g2, d["dh_in"])
    # t5_rmsnorm alone, module forward
    hl = h2.detach().clone().requires_grad_()
    gh, gw2 = torch.autograd.grad(m(hl), [hl, m.weight], d["dy"])
    assert torch.equal(gw2, gw) and torch.equal(gh, g1)


def test_frozen_weight_no_workspace_and_no_grad_keeps_nothing():
    N, D, dtype = 4096, 768, torch.bfloat16
    d = on_device(C.case(N, D, dtype, special=False))
    x, r = d["x"].requires_grad_(), d["residual"]
    w = d["w"]                                                   # frozen
    row = N * D * 2
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    h, y = P.t5_add_rmsnorm(x, r, w)
    assert torch.cuda.memory_allocated() - base <= 2 * row + 2 * (N * 4 + 512)          # h, y, rstd
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (gx,) = torch.autograd.grad(y, x, d["dy"])
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= row + 1024                       # dh alone: no partials
    del h, y, gx
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        h, y = P.t5_add_rmsnorm(x, r, w)
        y1 = P.t5_rmsnorm(x, w)
    assert torch.cuda.memory_allocated() - base == 3 * row      # no rstd kept
    assert h.grad_fn is None and y.grad_fn is None and y1.grad_fn is None


def test_forward_backward_peak_memory_is_below_hf_eager():
    N, D, dtype = 4096, 768, torch.bfloat16
    d = on_device(C.case(N, D, dtype, special=False))
    peaks = {}
    for route in ("fused", "hf_eager"):
        x, r, w = (d[k].clone().requires_grad_() for k in ("x", "residual", "w"))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if route == "fused":
            h, y = P.t5_add_rmsnorm(x, r, w)
        else:
            h = r + x
            y = C.hf_norm(h, w)
        grads = torch.autograd.grad([h, y], [x, r, w], [d["dh_in"], d["dy"]])
        torch.cuda.synchronize()
        peaks[route] = torch.cuda.max_memory_allocated() - base
        del h, y, grads
    print("forward + backward peak rise, bytes:", peaks)
    MEMORY.update({"shape": [N, D], "dtype": "bf16", "forward_backward_peak_rise_bytes": peaks})
    assert peaks["fused"] < peaks["hf_eager"]


# ------------------------------------------------------------------ refusals on the device
def test_argument_errors_leave_the_outputs_untouched():
    N, D, dtype = 5, 64, torch.bfloat16
    d = on_device(C.case(N, D, dtype))
    y = torch.full((N, D), SENTINEL, dtype=dtype, device=DEV)
    h = torch.full((N, D), SENTINEL, dtype=dtype, device=DEV)
    dh = torch.full((N, D), SENTINEL, dtype=dtype, device=DEV)
    dw = torch.full((D,), SENTINEL, dtype=dtype, device=DEV)
    ws = torch.full((P.t5_norm.geometry(N, D)["ws_bytes"] // 4,), SENTINEL, dtype=torch.float32, device=DEV)
    wide = torch.zeros(2, GEO["max_d"] + 8, dtype=dtype, device=DEV)
    f = dict(w=d["w"], x=d["x"], residual=d["residual"], h=h, y=y)

    def short(t):                                                # the same rows with a row stride below D
        return t.as_strided((N, D), (D // 2, 1))

    b = dict(w=d["w"], dw=dw, ws=ws, h=d["x"], dy=d["dy"], dh=dh)
    cases = [("trlx_t5_rmsnorm_fwd", {**f, "x": None}, 5), ("trlx_t5_rmsnorm_fwd", {**f, "w": None}, 5),
             ("trlx_t5_rmsnorm_fwd", {**f, "h": None}, 5), ("trlx_t5_rmsnorm_fwd", {**f, "y": h}, 5),
             ("trlx_t5_rmsnorm_fwd", {**f, "y": h[:, 8:]}, 5),
             ("trlx_t5_rmsnorm_fwd", {**f, "x": short(d["x"])}, 2), ("trlx_t5_rmsnorm_fwd", {**f, "y": short(y)}, 2),
             ("trlx_t5_rmsnorm_bwd", {**b, "dy": None}, 5), ("trlx_t5_rmsnorm_bwd", {**b, "dh": None, "dw": None, "ws": None}, 5),
             ("trlx_t5_rmsnorm_bwd", {**b, "ws": ws[:-1]}, 5), ("trlx_t5_rmsnorm_bwd", {**b, "ws": None}, 5),
             ("trlx_t5_rmsnorm_bwd", {**b, "dh": short(dh)}, 2), ("trlx_t5_rmsnorm_bwd", {**b, "dh": d["x"]}, 5)]
    for entry, ops, status in cases:
        with pytest.raises(ValueError, match=rf"status {status}"):
            call(entry, N, D, dtype, **ops)
    bad = raw_args(N, D, dtype, **f)
    bad.dtype = _lib.I64
    with pytest.raises(ValueError, match="status 3"):
        _lib.call("trlx_t5_rmsnorm_fwd", ctypes.byref(bad), None)
    with pytest.raises(ValueError, match="status 1"):             # D over the limit
        call("trlx_t5_rmsnorm_fwd", 2, wide.shape[1], dtype, w=wide[0], x=wide, y=torch.empty_like(wide))
    torch.cuda.synchronize()
    for t in (y, h, dh, dw, ws):
        assert bool((t == SENTINEL).all())
    # over the limit the Python entry takes HF's expressions
    got = P.t5_rmsnorm(wide + 1, torch.ones(wide.shape[1], dtype=dtype, device=DEV))
    assert torch.equal(got, C.hf_norm(wide + 1, torch.ones(wide.shape[1], dtype=dtype, device=DEV)))
