"""fp8 weights for the decode-step projections on the GPU (csrc/t5_decode_linear_w8.hip):
t5_quantize_linear_weight against torch's cast, t5_decode_linear_w8 against the float64 oracle and
t5_decode_linear on its own dequantize(), and t5_decode_layer_fused on a T5DecodeBlockWeights8.

The accuracy rule is t5_decode_linear_checks': with (b) the float64 oracle on w8.dequantize() and (a)
t5_decode_linear on w8.dequantize(), max|kernel - (b)| <= 2 max|(a) - (b)| + one bf16 ulp of max|(b)|.
Measured on the MI355X the worst ratio per combination is in profiles/t5_decode_linear_w8_parity.json
(tools/t5_decode_linear_w8_bench.py --parity runs these shapes)."""
import pytest
import torch

import trlx_t5_amd as P
import t5_cross_kv8_checks as C
import t5_decode_linear_checks as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
WAVES = (4, 8, 16)
MS = (1, 16, 17, 33)


def w8_shapes(norm, gated):
    """(waves, M, N, K).  Per WV the K at which the kernel takes another path: a partial turn, one turn,
    the second wave's first work, every wave busy, wave 0's second turn, the double buffer's steady
    state; then every row-tile count and a second pass at K 320; N 48 once."""
    out = []
    for wv in WAVES:
        ks = (64, 192, 256, 320, 256 * wv, 256 * wv + 64, 512 * wv + 64)
        out += [(wv, MS[i % 4], 16, k) for i, k in enumerate(ks) if not norm or k <= L.NORM_MAX_K]
        out += [(wv, m, 16, 320) for m in L.M_BREAKS]
    return out + [(8, 17, 48, 320)]


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------ quantiser
def special_weight(N, K):
    """A packed [3N, K] bf16 weight whose middle slice holds: row 0 zero, row 1 scaled by 1e30, row 2 by
    1e-30, row 3 the exact ties of the cast under scale 1, row 4 an Inf (the non-finite rule)."""
    w = torch.randn(3 * N, K, generator=torch.Generator().manual_seed(N + K))
    mid = w[N:2 * N]
    mid[0] = 0.0
    mid[1] *= 1e30
    mid[2] *= 1e-30
    mid[3] = 0.0
    mid[3, :len(C.TIES)] = torch.tensor([v for v, _ in C.TIES])
    mid[3, K - 1] = -448.0
    mid[4, K // 2] = float("inf")
    return w.to(BF)


@pytest.mark.parametrize("N,K", ((16, 64), (48, 320), (16, 4160)))
def test_quantiser_bytes_and_scales_are_torchs_bit_for_bit(N, K):
    packed = special_weight(N, K)
    want8, want_scale = C.ref_quantize(packed[N:2 * N][None, :, None, :])
    got = P.t5_quantize_linear_weight(packed.to(DEV)[N:2 * N])          # rows read through the packed stride
    assert got.shape == (N, K) and got.w8.dtype == torch.float8_e4m3fn and got.w8.is_contiguous()
    assert torch.equal(got.w8.view(torch.uint8).cpu(), want8[0, :, 0])
    assert C.same_scales(got.scale, want_scale[0])
    assert float(got.scale[0]) == 1.0 and not got.w8.view(torch.uint8)[0].any()              # the zero row
    assert float(got.scale[3]) == 1.0 and torch.equal(got.w8[3, :len(C.TIES)].float().cpu(), torch.tensor([k for _, k in C.TIES]))
    assert torch.isnan(got.scale[4]) and (got.w8.view(torch.uint8)[4] == 0x7f).all()          # the non-finite row
    ok = torch.isfinite(got.scale)
    exact = got.w8.float().double() * got.scale.double()[:, None]
    assert torch.equal(got.dequantize().double()[ok], exact[ok])                              # dequantize() is exact
    again = P.t5_quantize_linear_weight(packed.to(DEV)[N:2 * N], out=got)
    assert again is got and torch.equal(got.w8.view(torch.uint8).cpu(), want8[0, :, 0])


# ------------------------------------------------------------------ accuracy, determinism
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_name)
def test_accuracy_against_the_oracle_on_the_dequantised_weight_and_two_calls_agree(combo):
    norm, (_, with_res, act, gated) = combo
    worst = 0.0
    for wv, M, N, K in w8_shapes(norm, gated):
        x, w, nw, res = L.inputs(M, N, K, gated, seed=1000 * K + 10 * N + M, device=DEV)
        w8 = P.t5_quantize_linear_weight(w)
        wd = w8.dequantize()
        kw = dict(norm_weight=nw if norm else None, residual=res if with_res else None, act=act, gated=gated)
        ref = L.oracle(x, wd, kw["norm_weight"], 1e-6, kw["residual"], act, gated)
        e_bf16 = L.max_err(P.t5_decode_linear(x, wd, **kw), ref)
        out = P.t5_decode_linear_w8(x, w8, waves=wv, **kw)
        e_kernel = L.max_err(out, ref)
        limit = L.bound(e_bf16, ref)
        print(f"{L.combo_name(combo)} WV {wv} M {M} N {N} K {K}: e_kernel {e_kernel:.4g} e_bf16 {e_bf16:.4g} "
              f"bound {limit:.4g} ratio {e_kernel / limit:.3f}")
        worst = max(worst, e_kernel / limit)
        assert torch.isfinite(out.float()).all() and e_kernel <= limit, (wv, M, N, K, e_kernel, e_bf16, limit)
        assert torch.equal(bits(out), bits(P.t5_decode_linear_w8(x, w8, waves=wv, **kw))), (wv, M, N, K, "two calls differ")
    print(f"{L.combo_name(combo)}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("wv", WAVES)
def test_a_rows_bits_do_not_depend_on_the_other_rows_or_on_n(wv):
    K = 512 * wv + 64
    x, w, nw, _ = L.inputs(33, 48, K, False, seed=wv, device=DEV)
    w8 = P.t5_quantize_linear_weight(w)
    full = P.t5_decode_linear_w8(x, w8, norm_weight=nw if K <= L.NORM_MAX_K else None, waves=wv)
    part8 = P.T5LinearW8(w8.w8[16:32].clone(), w8.scale[16:32].clone())
    for m in (0, 1, 16, 32):
        alone = P.t5_decode_linear_w8(x[m:m + 1], part8, norm_weight=nw if K <= L.NORM_MAX_K else None, waves=wv)
        assert torch.equal(bits(alone[0]), bits(full[m, 16:32])), m
    assert torch.equal(bits(P.t5_decode_linear_w8(x, w8, waves=None)),
                       bits(P.t5_decode_linear_w8(x, w8, waves=P.t5_linear_w8.linear_w8_geometry(48, K)["waves"])))


def test_a_rows_scale_is_applied_exactly():
    """One weight row times 2^7: the same bytes, a scale 2^7 larger, and that output column is 2^7
    times the other run's, bit for bit (bf16 rounding of normal numbers commutes with a power of two;
    the inputs keep every output normal)."""
    x, w, _, _ = L.inputs(17, 16, 576, False, seed=7, device=DEV)
    w2 = w.clone()
    w2[5] = (w2[5].float() * 128.0).to(BF)
    a, b = P.t5_quantize_linear_weight(w), P.t5_quantize_linear_weight(w2)
    assert torch.equal(a.w8.view(torch.uint8), b.w8.view(torch.uint8))
    assert torch.equal(b.scale[5], a.scale[5] * 128.0) and torch.equal(torch.cat([a.scale[:5], a.scale[6:]]), torch.cat([b.scale[:5], b.scale[6:]]))
    ya, yb = P.t5_decode_linear_w8(x, a), P.t5_decode_linear_w8(x, b)
    assert torch.equal(bits(torch.ldexp(ya[:, 5].float(), torch.tensor(7, device=DEV)).to(BF)), bits(yb[:, 5]))
    keep = [c for c in range(16) if c != 5]
    assert torch.equal(bits(ya[:, keep]), bits(yb[:, keep]))


# ------------------------------------------------------------------ the layer
@pytest.mark.parametrize("gated", (True, False), ids=("gated", "plain"))
def test_the_fused_layer_on_fp8_weights_is_the_chain_of_its_calls(gated):
    D, inner, F = 128, 128, 256
    sd = {k: v.to(DEV) for k, v in L.hf_block_state_dict(D, inner, F, gated, seed=11).items()}
    w = P.T5DecodeBlockWeights8.from_state_dict(sd, "decoder.block.0.", gated=gated)
    bf = P.T5DecodeBlockWeights.from_state_dict(sd, "decoder.block.0.", gated=gated)
    assert torch.equal(w.qkv.w8.view(torch.uint8), P.t5_quantize_linear_weight(bf.qkv).w8.view(torch.uint8))
    assert all(torch.equal(a, b) for a, b in zip(w.ln, bf.ln)) and (w.inner, w.d_model, w.d_ff) == (inner, D, F)
    h0 = torch.randn(9, D, generator=torch.Generator().manual_seed(3)).to(BF).to(DEV)
    sa = lambda q, k, v: (q.float() + k.float() - v.float()).to(q.dtype)
    ca = lambda q: (q.float() * 0.5).to(q.dtype)
    h = h0.clone()
    assert P.t5_decode_layer_fused(h, w, sa, ca, act="silu") is h
    lin = P.t5_decode_linear_w8
    qkv = lin(h0, w.qkv, norm_weight=w.ln[0])
    want = lin(sa(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:]), w.o, residual=h0)
    want = lin(ca(lin(want, w.cq, norm_weight=w.ln[1])), w.co, residual=want)
    want = lin(lin(want, w.wi, norm_weight=w.ln[2], act="silu", gated=gated), w.wo, residual=want)
    assert torch.equal(bits(h), bits(want))
    with pytest.raises(ValueError, match="no rows form"):
        P.t5_decode_layer_fused(h, w, sa, ca, split_rows=True)


# ------------------------------------------------------------------ refusals
def test_refusals_carry_their_reason():
    x, w, nw, _ = L.inputs(3, 16, 128, False, seed=1, device=DEV)
    w8 = P.t5_quantize_linear_weight(w)
    for bad_k in (96, 16448):
        xb, wb, _, _ = L.inputs(3, 16, bad_k, False, seed=2, device=DEV)
        with pytest.raises(ValueError, match="multiple of 64, at most 16384"):
            P.t5_decode_linear_w8(xb, P.T5LinearW8(wb.to(torch.float8_e4m3fn), torch.ones(16, device=DEV)))
    with pytest.raises(ValueError, match="multiple of 16"):
        P.t5_decode_linear_w8(x, P.T5LinearW8(w8.w8[:8].clone(), w8.scale[:8].clone()))
    xk, wk, nwk, _ = L.inputs(2, 16, 8256, False, seed=3, device=DEV)
    with pytest.raises(ValueError, match="t5_rmsnorm's limit"):
        P.t5_decode_linear_w8(xk, P.t5_quantize_linear_weight(wk), norm_weight=nwk)
    with pytest.raises(ValueError, match="no fp32 form"):
        P.t5_decode_linear_w8(x.float(), w8)
    with pytest.raises(ValueError, match="waves"):
        P.t5_decode_linear_w8(x, w8, waves=2)
    with pytest.raises(ValueError, match="scale must be"):
        P.T5LinearW8(w8.w8, w8.scale[:8])
    with pytest.raises(TypeError):
        P.t5_decode_linear_w8(x, w)
