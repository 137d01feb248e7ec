"""The grouped decode cross-attention on the GPU (trlx_t5_decode_attn_group, k_t5_decode_attn_group;
t5_decode_cross_attention_grouped) against the existing kernel on the expanded tensors.

Every comparison with the existing kernel is equality of the raw bits: per query the grouped kernel
executes that kernel's floating-point operations in that kernel's order, so a difference is a drift
of the arithmetic, never a tolerance.  The float64 oracle and torch's eager route supply a second
yardstick that is not this project's own kernel.  Rows the call must not read hold NaN."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_cross_group_checks as G
import t5_decode_attn_checks as A
import t5_rollout_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GEOMETRIES = [(dt, d) for dt in A.DTYPES for d in A.D_KVS]
GEOMETRY_IDS = [f"{A.dtype_name(dt)}-d{d}" for dt, d in GEOMETRIES]
grouped = P.t5_decode_cross_attention_grouped


def dev(x):
    return None if x is None else x.to(DEV)


def expanded_call(q, K, V, mask, Gn, live=None):
    """The existing kernel on the repeat_interleave'd operands: what every row is held to."""
    return P.t5_decode_cross_attention(q, G.expand(K, Gn), G.expand(V, Gn), G.expand(mask, Gn), live=live)


def nan_rows(x, rows):
    x = x.clone()
    x[rows] = float("nan")
    return x


# ------------------------------------------------------------------ 1. the bits of the existing kernel
@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_every_row_has_the_bits_of_the_existing_kernel_on_the_expanded_tensors(dtype, d):
    for S in G.cross_s(dtype, d):
        for kind in A.MASKS:
            c = A.cross_case(dtype, d, S, kind)
            K, V, mask = dev(c["K"]), dev(c["V"]), dev(c["mask"])
            for Gn in G.GS:
                q = dev(G.group_q(dtype, d, S, kind, Gn))
                got = grouped(q, K, V, mask)
                assert got.dtype == dtype and tuple(got.shape) == (G.P * Gn, G.NH * d) and got.is_contiguous()
                assert C.same(got, expanded_call(q, K, V, mask, Gn)), (S, kind, Gn)


@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_the_result_does_not_depend_on_the_query_tile(dtype, d):
    """Every built tile, also the ones the entry would not pick for this G, gives the same bits."""
    ng = G.groups(dtype, d)
    try:
        for S, kind in ((2 * ng + 1, "holes"), (33, "none")):
            c = A.cross_case(dtype, d, S, kind)
            K, V, mask = dev(c["K"]), dev(c["V"]), dev(c["mask"])
            for Gn in (1, 3, 5, 8, 9):
                q = dev(G.group_q(dtype, d, S, kind, Gn))
                want = expanded_call(q, K, V, mask, Gn)
                for tile in G.TILES:
                    P.t5_decode.t5_decode_cross_attention_group_tile(tile)
                    assert C.same(grouped(q, K, V, mask), want), (S, kind, Gn, tile)
    finally:
        P.t5_decode.t5_decode_cross_attention_group_tile(0)


# ------------------------------------------------------------------ 2. a yardstick that is not this project
@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_the_error_against_the_float64_oracle_is_within_torchs_own(dtype, d):
    """max|kernel - oracle| <= bound(max|eager - oracle|): t5_decode_attn_checks' rule, unchanged.  The
    oracle and torch's eager route see the expanded tensors; the kernel sees the shared ones with NaN
    in the masked rows."""
    ng = G.groups(dtype, d)
    for S in (9, 2 * ng + 1, 200):
        for kind in A.MASKS:
            c = A.cross_case(dtype, d, S, kind)
            Kp, Vp = A.poison(c["K"], c["mask"]), A.poison(c["V"], c["mask"])
            for Gn in (4, 5):
                q = G.group_q(dtype, d, S, kind, Gn)
                q3 = q.reshape(G.P * Gn, G.NH, d)
                want = A.oracle_cross(q3, G.expand(Kp, Gn), G.expand(Vp, Gn), G.expand(c["mask"], Gn))
                eager = A.eager_cross(dev(q3), dev(G.expand(c["K"], Gn)), dev(G.expand(c["V"], Gn)),
                                      dev(G.expand(c["mask"], Gn)))
                got = grouped(dev(q), dev(Kp), dev(Vp), dev(c["mask"]))
                e_k, e_t = A.max_err(got, want), A.max_err(eager, want)
                lim = A.bound(dtype, e_t, want)
                fig = dict(dtype=A.dtype_name(dtype), d_kv=d, S=S, mask=kind, G=Gn, e_torch=e_t, e_kernel=e_k, bound=lim)
                print(fig)
                assert torch.isfinite(got).all() and e_k <= lim, fig


# ------------------------------------------------------------------ 3. layouts
@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_layouts_are_read_in_place_and_give_the_same_bits(dtype, d, monkeypatch):
    S, kind, Gn = 33, "holes", 5
    c = G.group_case(dtype, d, S, kind, Gn)
    inner = G.NH * d
    q, K, V, mask = dev(c["q"]), dev(c["K"]), dev(c["V"]), dev(c["mask"])
    want = grouped(q, K, V, mask)
    assert C.same(want, expanded_call(q, K, V, mask, Gn))
    seen = []
    real = _lib.call

    def spy(name, *a):
        if name == "trlx_t5_decode_attn_group":
            s = a[0]._obj
            seen.append((s.q, s.ldq, s.k, s.k_stride_p, s.k_stride_h, s.k_stride_s, s.v, s.v_stride_p, s.v_stride_h,
                         s.v_stride_s))
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    # the projection output [P, S, nH * d], as the host holds it
    k_host = c["K"].permute(0, 2, 1, 3).reshape(G.P, S, inner).contiguous()
    v_host = c["V"].permute(0, 2, 1, 3).reshape(G.P, S, inner).contiguous()
    k3, v3 = k_host.to(DEV), v_host.to(DEV)
    assert k3.stride() == k_host.stride() == (S * inner, inner, 1) and v3.stride() == v_host.stride()
    assert C.same(grouped(q, k3, v3, mask, n_heads=G.NH), want)
    assert seen[-1] == (q.data_ptr(), inner, k3.data_ptr(), S * inner, d, inner, v3.data_ptr(), S * inner, d, inner)
    # HF's transposed view of it
    assert C.same(grouped(q, k3.view(G.P, S, G.NH, d).transpose(1, 2), v3.view(G.P, S, G.NH, d).transpose(1, 2), mask), want)
    assert seen[-1][2:] == (k3.data_ptr(), S * inner, d, inner, v3.data_ptr(), S * inner, d, inner)
    # K and V of different layouts in one call
    assert C.same(grouped(q, K, v3.view(G.P, S, G.NH, d).transpose(1, 2), mask), want)
    # q as a slice of a fused projection, and as [P * G, 1, nH * d]
    qkv = torch.full((G.P * Gn, 3 * inner), float("nan"), dtype=dtype, device=DEV)
    qkv[:, inner:2 * inner] = q
    assert C.same(grouped(qkv[:, inner:2 * inner], K, V, mask), want)
    assert seen[-1][:2] == (qkv.data_ptr() + inner * qkv.element_size(), 3 * inner)
    assert C.same(grouped(q[:, None, :], K, V, mask), want)
    assert C.same(grouped(q.reshape(G.P * Gn, G.NH, d), K, V, mask), want)
    # strides the kernel does not take are copied once, not refused
    wide = torch.zeros(G.P, G.NH, S, d + 1, dtype=dtype, device=DEV)
    wide[..., :d] = K
    assert C.same(grouped(q, wide[..., :d], V, mask), want)


# ------------------------------------------------------------------ 4. nothing read that should not be
@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_dead_rows_masked_keys_and_dead_prompts_are_not_read(dtype, d):
    ng = G.groups(dtype, d)
    for S, kind in ((2 * ng + 1, "holes"), (ng - 1, "right"), (9, "none")):
        c = A.cross_case(dtype, d, S, kind)
        mask = dev(c["mask"])
        K, V = dev(c["K"]), dev(c["V"])
        Kp, Vp = dev(A.poison(c["K"], c["mask"])), dev(A.poison(c["V"], c["mask"]))    # NaN in the masked rows
        for Gn in G.GS:
            q = dev(G.group_q(dtype, d, S, kind, Gn))
            want = grouped(q, K, V, mask)
            assert torch.isfinite(want.float()).all()
            assert C.same(grouped(q, Kp, Vp, mask), want), (S, kind, Gn, "masked rows")
            for name, pattern in G.live_sets(Gn).items():
                live = dev(pattern)
                on = live != 0
                dead_prompts = ~on.view(G.P, Gn).any(dim=1)
                got = grouped(nan_rows(q, ~on), nan_rows(Kp, dead_prompts), nan_rows(Vp, dead_prompts), mask, live=live)
                assert not torch.isnan(got.float()).any(), (S, kind, Gn, name)
                assert C.same(got[on], want[on]), (S, kind, Gn, name, "live rows")
                assert C.same(got[~on], torch.zeros_like(got[~on])), (S, kind, Gn, name, "dead rows")
                assert live.tolist() == pattern.tolist()
                if name == "all_live":
                    assert C.same(got, want)


@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_a_fully_masked_prompt_gives_zeros_in_all_its_rows(dtype, d):
    S, Gn = 2 * G.groups(dtype, d) + 1, 5
    c = G.group_case(dtype, d, S, "holes", Gn)
    mask = c["mask"].clone()
    mask[1] = 0
    q, mdev = dev(c["q"]), dev(mask)
    got = grouped(q, dev(A.poison(c["K"], mask)), dev(A.poison(c["V"], mask)), mdev)
    assert C.same(got, expanded_call(q, dev(c["K"]), dev(c["V"]), mdev, Gn))
    assert not got[Gn:2 * Gn].any() and got[:Gn].any() and got[2 * Gn:].any() and not torch.isnan(got.float()).any()


# ------------------------------------------------------------------ 5. guard words around out
def entry(tq, tk, tv, tmask, tlive, tout, Gn, **over):
    """trlx_t5_decode_attn_group itself on contiguous device tensors, fields replaced by `over`; returns
    the status."""
    Pn, nH, S, d = tk.shape
    a = _lib.T5DecodeAttnGroupArgs(
        q=tq.data_ptr(), ldq=tq.stride(0), k=tk.data_ptr(), k_stride_p=tk.stride(0), k_stride_h=tk.stride(1),
        k_stride_s=tk.stride(2), v=tv.data_ptr(), v_stride_p=tv.stride(0), v_stride_h=tv.stride(1),
        v_stride_s=tv.stride(2), key_mask=_lib.ptr(tmask), live=_lib.ptr(tlive), out=tout.data_ptr(), P=Pn, G=Gn,
        n_heads=nH, d_kv=d, S=S, dtype=_lib.dtype_code(tk))
    for k, v in over.items():
        setattr(a, k, v)
    return _lib.query("trlx_t5_decode_attn_group", ctypes.byref(a), _lib.stream_of(tout))


@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=GEOMETRY_IDS)
def test_nothing_is_written_before_or_after_out(dtype, d):
    S, kind = 33, "left"
    c = A.cross_case(dtype, d, S, kind)
    K, V, mask = dev(c["K"]), dev(c["V"]), dev(c["mask"])
    inner = G.NH * d
    for Gn in (4, 5, 9):                                           # a whole tile and two remainder tiles
        q = dev(G.group_q(dtype, d, S, kind, Gn))
        for live in (None, dev(G.live_sets(Gn)["alternating"]), dev(G.live_sets(Gn)["all_dead"])):
            whole, out = C.with_margins((G.P * Gn, inner), dtype, DEV, inner)
            assert entry(q, K, V, mask, live, out, Gn) == 0
            torch.cuda.synchronize()
            assert C.same(out, grouped(q, K, V, mask, live=live)), (Gn, live is None)
            lo = C.MARGIN * inner
            edge = torch.full((lo,), C.GUARD, dtype=dtype, device=DEV)
            assert C.same(whole[:lo], edge) and C.same(whole[lo + G.P * Gn * inner:], edge), (Gn, live is None)


# ------------------------------------------------------------------ 6. one capture, live rewritten
def test_one_captured_call_replays_with_live_rewritten():
    dtype, d, Gn = torch.bfloat16, 64, 5
    S = 2 * G.groups(dtype, d) + 1
    c = G.group_case(dtype, d, S, "holes", Gn)
    q, K, V, mask = dev(c["q"]), dev(c["K"]), dev(c["V"]), dev(c["mask"])
    sets = G.live_sets(Gn)
    patterns = [sets[k] for k in ("alternating", "one_prompt_dead", "last_row_of_each_prompt", "all_live")]
    want = [grouped(q, K, V, mask, live=dev(p)) for p in patterns]
    live = torch.ones(G.P * Gn, dtype=torch.int64, device=DEV)
    grouped(q, K, V, mask, live=live)                              # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one stream, one launch, no branches
        out = grouped(q, K, V, mask, live=live)
    for p, w in zip(patterns, want):
        live.copy_(dev(p))
        graph.replay()
        torch.cuda.synchronize()
        assert C.same(out, w), p.tolist()


# ------------------------------------------------------------------ 7. refusals on device tensors
def test_refusals_leave_out_untouched():
    dtype, d, S, Gn = torch.bfloat16, 64, 9, 4
    c = G.group_case(dtype, d, S, "right", Gn)
    q, K, V, mask = dev(c["q"]), dev(c["K"]), dev(c["V"]), dev(c["mask"])
    n, inner = G.P * Gn, G.NH * d
    with pytest.raises(ValueError, match="whole multiple"):
        grouped(q[:-1], K, V, mask)
    with pytest.raises(ValueError, match="key_mask"):
        grouped(q, K, V, G.expand(mask, Gn))
    with pytest.raises(ValueError, match="key_mask"):
        grouped(q, K, V, mask.cpu())
    with pytest.raises(ValueError):
        grouped(q.cpu(), K, V, mask)
    with pytest.raises(ValueError):
        grouped(q, K, V.float(), mask)
    with pytest.raises(ValueError, match="n_heads"):
        grouped(q, K.transpose(1, 2).reshape(G.P, S, inner), V.transpose(1, 2).reshape(G.P, S, inner), mask)
    for live in (torch.ones(n, dtype=torch.int64), torch.ones(n, dtype=torch.int32, device=DEV),
                 torch.ones(G.P, dtype=torch.int64, device=DEV), torch.ones(2 * n, dtype=torch.int64, device=DEV)[::2]):
        with pytest.raises(ValueError, match="live"):
            grouped(q, K, V, mask, live=live)
    # the C entry on device memory
    live = torch.ones(n + 1, dtype=torch.int64, device=DEV)
    out = torch.full((n, inner), C.GUARD, dtype=dtype, device=DEV)
    for over in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(dtype=_lib.I64), dict(d_kv=32),
                 dict(P=0), dict(G=0), dict(n_heads=0), dict(S=0), dict(ldq=inner - 8), dict(ldq=inner + 4),
                 dict(k_stride_p=-K.stride(0)), dict(v_stride_s=d + 4), dict(k_stride_h=d - 8), dict(v_stride_s=d - 8),
                 dict(q=q.data_ptr() + 2), dict(k=K.data_ptr() + 8), dict(v=V.data_ptr() + 4),
                 dict(out=out.data_ptr() + 2), dict(key_mask=mask.data_ptr() + 4), dict(live=live.data_ptr() + 4),
                 dict(P=1 << 33), dict(P=1, G=1 << 20)):
        assert entry(q, K, V, mask, live, out, Gn, **over) == C.ERR_ARG, over
    assert _lib.query("trlx_t5_decode_attn_group", None, _lib.stream_of(out)) == C.ERR_ARG
    torch.cuda.synchronize()
    assert C.same(out, torch.full_like(out, C.GUARD))
    assert entry(q, K, V, mask, live[1:], out, Gn) == 0             # the same arguments, legal: it does run
    torch.cuda.synchronize()
    assert C.same(out, grouped(q, K, V, mask))
