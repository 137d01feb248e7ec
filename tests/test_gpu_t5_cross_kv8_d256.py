"""The fp8 encoder keys / values at d_kv 256 (the UL2 head size) on the GPU: trlx_t5_cross_kv_quantize
at 256 against the CPU restatement, bit for bit, and trlx_t5_decode_attn_kv8_d256 -- a kernel of its
own, the keys optionally cut across workgroups -- against the float64 oracle on the DEQUANTISED keys
and values under the bf16 kernel's rule (t5_decode_attn_checks.bound):
    max|kernel - oracle| <= max|eager - oracle| + one bf16 ulp of max|oracle|
with eager = torch's own route on the device, fed the dequantised bf16 tensors.

ATTN_S holds the S of the bf16 tests and both sides of every break the geometry helper reports: the
rows of a wave-wide load, the lane groups, the keys of a trip, the keys of a range at 2 and 3 splits.
S = 1 leaves every range but the first empty."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_decode_attn_checks as A
import t5_cross_kv8_checks as C
from t5_rollout_checks import ERR_ARG, GUARD, same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
D = 256
SPLITS = (1, 2, 3)
GEO = {x: P.t5_decode_cross_attention_kv8_d256_geometry(A.CROSS_S[-1], x) for x in SPLITS}
BREAKS = {GEO[1][k] for k in ("rows_per_wave_load", "lane_groups", "keys_per_trip")} | {GEO[x]["keys_per_range"] for x in (2, 3)}
ATTN_S = tuple(sorted(set(A.CROSS_S) | {e + o for e in BREAKS for o in (-1, 0, 1)}))
TRIP, RANGE2 = GEO[1]["keys_per_trip"], GEO[2]["keys_per_range"]
_ATTN = {}


def dev(x):
    return None if x is None else x.to(DEV)


def quantised(want):
    return want.k8.view(torch.uint8), want.k_scale, want.v8.view(torch.uint8), want.v_scale


def attn_case(S, kind, mask=None):
    """cross_case quantised on the device (once per case), with the oracle and the eager error."""
    key = (S, kind, mask is not None)
    if key not in _ATTN:
        c = A.cross_case(BF, D, S, kind)
        mask = c["mask"] if mask is None else mask
        kv8 = P.t5_quantize_cross_kv(dev(A.poison(c["K"], mask)), dev(A.poison(c["V"], mask)), dev(mask))
        Kd, Vd = kv8.dequantize()
        ref = A.oracle_cross(c["q"], Kd.cpu(), Vd.cpu(), mask)
        eager = A.eager_cross(dev(c["q"]), Kd, Vd, dev(mask))
        assert torch.isfinite(eager.float()).all()
        _ATTN[key] = dict(q=dev(c["q"]), mask=dev(mask), kv8=kv8, ref=ref, eager=eager, e_torch=A.max_err(eager, ref))
    return _ATTN[key]


# ------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("kind", A.MASKS)
def test_quantiser_equals_the_cpu_restatement(kind):
    for S in C.QUANT_S:
        c = A.cross_case(BF, D, S, kind)
        K, V = A.poison(c["K"], c["mask"]), A.poison(c["V"], c["mask"])   # masked rows are not read
        want = quantised(P.t5_quantize_cross_kv(K, V, c["mask"]))
        for name, (k_in, nh) in C.layouts(K).items():
            got = P.t5_quantize_cross_kv(dev(k_in), dev(C.layouts(V)[name][0]), dev(c["mask"]), n_heads=nh)
            assert got.k8.is_cuda and got.d_kv == D and C.quantised_equal(got, *want), (S, name)


def test_quantiser_special_values_and_a_non_finite_block():
    c = C.special_case(D)
    got = P.t5_quantize_cross_kv(dev(c["K"]), dev(c["V"]), dev(c["mask"]))
    assert C.quantised_equal(got, *quantised(P.t5_quantize_cross_kv(c["K"], c["V"], c["mask"])))
    assert float(got.k_scale[0, 0]) == 1.0 and not got.k8.view(torch.uint8)[1].any()
    assert torch.equal(got.k8[0, 0, 0, :len(C.TIES)].float().cpu(), torch.tensor([w for _, w in C.TIES]))
    c = A.cross_case(BF, D, RANGE2 + 1, "holes")           # two ranges at 2 and 3 splits
    K, V = c["K"].clone(), c["V"].clone()
    K[1, 2, int(torch.nonzero(c["mask"][1])[0]), 3] = float("inf")
    V[0, 4, int(torch.nonzero(c["mask"][0])[-1]), 0] = float("nan")
    got = P.t5_quantize_cross_kv(dev(K), dev(V), dev(c["mask"]))
    assert C.quantised_equal(got, *quantised(P.t5_quantize_cross_kv(K, V, c["mask"])))
    for x in SPLITS:   # NaN for that (row, head) and no other
        out = P.t5_decode_cross_attention_kv8(dev(c["q"]), got, dev(c["mask"]), splits=x).view(C.B, C.NH, D).float().cpu()
        nan = torch.isnan(out).all(dim=2)
        assert nan[1, 2] and nan[0, 4] and nan.sum() == 2 and torch.isfinite(out[~nan]).all(), x


# ------------------------------------------------------------------ the attention
@pytest.mark.parametrize("kind", A.MASKS)
@pytest.mark.parametrize("splits", SPLITS)
def test_attention_against_the_oracle_on_the_dequantised_values(splits, kind):
    for S in ATTN_S:
        c = attn_case(S, kind)
        out = P.t5_decode_cross_attention_kv8(c["q"], c["kv8"], c["mask"], splits=splits)
        assert out.dtype == BF and out.shape == (C.B, C.NH * D)
        e_kernel, limit = A.max_err(out, c["ref"]), A.bound(BF, c["e_torch"], c["ref"])
        print(f"kv8 d256 splits {splits} S {S} {kind}: kernel {e_kernel:.3e} eager {c['e_torch']:.3e} bound {limit:.3e} "
              f"ratio {e_kernel / limit:.3f}")
        assert e_kernel <= limit, (S, e_kernel, limit)


@pytest.mark.parametrize("splits", SPLITS)
def test_a_dead_range_and_a_fully_masked_row(splits):
    S = A.CROSS_S[-1]
    mask = torch.ones(C.B, S, dtype=torch.int64)
    mask[0, :RANGE2 + 3] = 0          # left padding past the whole first range of two
    mask[1] = 0                       # no live key at all: zeros
    mask[2, RANGE2 - 5:] = 0          # the last range dead
    c = attn_case(S, "none", mask)
    out = P.t5_decode_cross_attention_kv8(c["q"], c["kv8"], c["mask"], splits=splits)
    assert not out[1].any() and out[0].any() and out[2].any() and torch.isfinite(out.float()).all()
    e_torch = A.max_err(c["eager"][[0, 2]], c["ref"][[0, 2]])
    assert A.max_err(out, c["ref"]) <= A.bound(BF, e_torch, c["ref"])


@pytest.mark.parametrize("splits", (1, 2))
def test_bits_repeat_and_do_not_depend_on_B_or_on_qs_stride(splits):
    for S in (33, RANGE2 + 1):
        c = attn_case(S, "holes")
        kv8, q, mask = c["kv8"], c["q"], c["mask"]
        out = P.t5_decode_cross_attention_kv8(q, kv8, mask, splits=splits)
        assert same(P.t5_decode_cross_attention_kv8(q, kv8, mask, splits=splits), out)
        inner = C.NH * D
        fused = torch.full((C.B, 3 * inner), float("nan"), dtype=BF, device=DEV)   # q as a slice of a qkv projection
        fused[:, inner:2 * inner] = q.reshape(C.B, inner)
        assert same(P.t5_decode_cross_attention_kv8(fused[:, inner:2 * inner], kv8, mask, splits=splits), out)
        assert same(P.t5_decode_cross_attention_kv8(q.reshape(C.B, C.NH, 1, D), kv8, mask, splits=splits), out)
        for b in range(C.B):                                                        # the same call at B = 1
            one = P.T5CrossKV8(1, C.NH, S, D, DEV)
            for dst, src in ((one.k8, kv8.k8), (one.v8, kv8.v8), (one.k_scale, kv8.k_scale), (one.v_scale, kv8.v_scale)):
                dst.copy_(src[b:b + 1])
            assert same(P.t5_decode_cross_attention_kv8(q[b:b + 1], one, mask[b:b + 1], splits=splits), out[b:b + 1]), (S, b)


def poisoned(kv8, q, on):
    """kv8 and q with the dead rows' bytes, scales and q poisoned."""
    bad = P.T5CrossKV8(kv8.B, kv8.n_heads, kv8.S, D, DEV)
    for dst, src in ((bad.k8, kv8.k8), (bad.v8, kv8.v8)):
        dst.view(torch.uint8).copy_(src.view(torch.uint8))
        dst.view(torch.uint8)[~on] = 0x7f
    for dst, src in ((bad.k_scale, kv8.k_scale), (bad.v_scale, kv8.v_scale)):
        dst.copy_(src)
        dst[~on] = float("nan")
    pq = q.clone()
    pq[~on] = float("nan")
    return bad, pq


@pytest.mark.parametrize("splits", (1, 2))
def test_live_skips_dead_rows_and_keeps_live_rows(splits):
    for S, kind in ((9, "none"), (TRIP + 1, "holes"), (RANGE2 + 1, "left")):
        c = attn_case(S, kind)
        want = P.t5_decode_cross_attention_kv8(c["q"], c["kv8"], c["mask"], splits=splits)
        for pattern in ([1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 0, 7]):
            live = torch.tensor(pattern, dtype=torch.int64, device=DEV)
            on = live != 0
            bad, pq = poisoned(c["kv8"], c["q"], on)
            ws = torch.full((P.t5_decode_cross_attention_kv8_d256_workspace_bytes(C.B, C.NH, splits) // 4,), float("nan"),
                            device=DEV)   # what the workspace held does not matter
            got = P.t5_decode_cross_attention_kv8(pq, bad, c["mask"], live=live, splits=splits, workspace=ws)
            assert same(got[on], want[on]), (S, pattern, "live rows")
            assert same(got[~on], torch.zeros_like(got[~on])), (S, pattern, "dead rows")
            assert live.tolist() == pattern


def test_one_captured_split_call_replays_with_live_rewritten():
    c = attn_case(RANGE2 + 1, "holes")
    kv8, q, mask = c["kv8"], c["q"], c["mask"]
    live = torch.ones(C.B, dtype=torch.int64, device=DEV)
    patterns = ([1, 1, 1], [1, 0, 1], [0, 0, 3])
    want = [P.t5_decode_cross_attention_kv8(q, kv8, mask, live=torch.tensor(p, dtype=torch.int64, device=DEV), splits=2)
            for p in patterns]                                          # eager: the workspace exists from here on
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = P.t5_decode_cross_attention_kv8(q, kv8, mask, live=live, splits=2)
    for p, w in zip(patterns, want):
        live.copy_(torch.tensor(p, dtype=torch.int64, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, w), p


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched():
    S = 9
    c = attn_case(S, "right")
    kv8, q, mask = c["kv8"], c["q"].reshape(C.B, C.NH * D), c["mask"]
    out = torch.full((C.B, C.NH * D), GUARD, dtype=BF, device=DEV)
    need = P.t5_decode_cross_attention_kv8_d256_workspace_bytes(C.B, C.NH, 2)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    stream = _lib.stream_of(out)
    ks, vs = kv8.k_scale.data_ptr(), kv8.v_scale.data_ptr()

    def attn(k_scale=ks, v_scale=vs, splits=1, ws_ptr=None, ws_bytes=0, **over):
        a = _lib.T5DecodeAttnArgs(
            q=q.data_ptr(), ldq=C.NH * D, k_new=None, ldk=0, v_new=None, ldv=0, k=kv8.k8.data_ptr(), v=kv8.v8.data_ptr(),
            bias_by_distance=None, key_mask=mask.data_ptr(), out=out.data_ptr(), B=C.B, n_heads=C.NH, d_kv=D, max_len=S,
            t=0, dtype=_lib.BF16, mode=_lib.T5_ATTN_CROSS)
        for k, v in over.items():
            setattr(a, k, v)
        return _lib.query("trlx_t5_decode_attn_kv8_d256", ctypes.byref(a), k_scale, v_scale, None, splits, ws_ptr, ws_bytes, stream)

    for kw in (dict(d_kv=128), dict(splits=0), dict(splits=17), dict(splits=2), dict(splits=2, ws_ptr=ws.data_ptr() + 8, ws_bytes=need),
               dict(splits=2, ws_ptr=ws.data_ptr(), ws_bytes=need - 4), dict(dtype=_lib.F32), dict(mode=_lib.T5_ATTN_SELF),
               dict(k_scale=None), dict(v_scale=None)):
        assert attn(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert same(out, torch.full_like(out, GUARD))
    assert attn() == 0 and attn(splits=2, ws_ptr=ws.data_ptr(), ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert same(out, P.t5_decode_cross_attention_kv8(q, kv8, mask, splits=2))
    k64 = P.T5CrossKV8(C.B, C.NH, S, 64, DEV)
    with pytest.raises(ValueError, match="splits"):
        P.t5_decode_cross_attention_kv8(q[:, :C.NH * 64], k64, mask, splits=2)
