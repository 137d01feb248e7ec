"""The grouped decode cross-attention on MFMA on the GPU (trlx_t5_decode_attn_group_mma:
k_t5_decode_attn_group_mma; t5_decode_cross_attention_grouped_mma).

The yardstick is the float64 oracle with torch's eager bf16 route on the device, under the rule
t5_attention lives by (the kernel rounds P to bf16 un-normalised as that one does):
max|kernel - oracle| <= 2 * e_torch + one bf16 ulp of max|oracle|.  Everything else is equality of
bits between two calls of the route.  Rows the call must not read hold NaN."""
import pytest
import torch

import trlx_t5_amd as P
import t5_cross_split_checks as S
import t5_decode_attn_checks as A
import t5_rollout_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
mma = P.t5_decode_cross_attention_grouped_mma
WAVES = {d: P.t5_decode.t5_decode_cross_attention_grouped_mma_waves(d) for d in A.D_KVS}
GS = (1, 7, 16, 17, 33)          # below a tile, a full tile, a remainder of one row after one and two tiles


def sizes(d):
    """Both sides of one 32-key block and of one round of all W waves, and 200."""
    w = WAVES[d]
    return sorted({1, 31, 32, 33, 32 * w - 1, 32 * w, 32 * w + 1, 200})


def dev(x):
    return None if x is None else x.to(DEV)


def case(d, Sn, kind, Gn):
    """q, K, V (NaN in the masked rows), mask on the device, and the CPU case."""
    c = S.group_case(BF, d, Sn, kind, Gn)
    return dev(c["q"]), dev(S.poison(c["K"], c["mask"])), dev(S.poison(c["V"], c["mask"])), dev(c["mask"]), c


def nan_rows(x, rows):
    x = x.clone()
    x[rows] = float("nan")
    return x


@pytest.mark.parametrize("d,Sn,Gn", [(d, Sn, Gn) for d in A.D_KVS for Sn in sizes(d) for Gn in GS])
def test_the_error_against_the_float64_oracle_is_within_twice_torchs_own(d, Sn, Gn):
    for kind in A.MASKS:
        want, e_t = S.reference(BF, d, Sn, kind, Gn, "cuda:0")
        q, K, V, mask, _ = case(d, Sn, kind, Gn)
        got = mma(q, K, V, mask)
        assert got.dtype == BF and tuple(got.shape) == (S.P * Gn, S.NH * d) and got.is_contiguous()
        e_k, lim = A.max_err(got, want), 2.0 * e_t + A.bf16_ulp(float(want.abs().max()))
        print(dict(d_kv=d, S=Sn, G=Gn, mask=kind, e_torch=e_t, e_kernel=e_k, bound=lim))
        assert torch.isfinite(got.float()).all() and e_k <= lim, (kind, e_k, lim)


@pytest.mark.parametrize("d", A.D_KVS)
def test_a_rows_bits_are_its_own(d):
    """Not the group size's, the tile place's, the K / V layout's or the q stride's."""
    Gn, Sn, inner = 17, 200, S.NH * d
    q, K, V, mask, c = case(d, Sn, "holes", Gn)
    want = mma(q, K, V, mask)
    assert C.same(mma(q, K, V, mask), want)
    last = mma(q[Gn - 1::Gn].contiguous(), K, V, mask)                # the remainder tile's one row, as a G 1 call
    assert C.same(last, want[Gn - 1::Gn])
    k3, v3 = (x.permute(0, 2, 1, 3).reshape(S.P, Sn, inner).contiguous() for x in (K, V))
    assert C.same(mma(q, k3, v3, mask, n_heads=S.NH), want)           # the projection output, read in place
    wide = torch.full((S.P * Gn, inner + 64), float("nan"), dtype=BF, device=DEV)
    wide[:, :inner] = q
    assert wide[:, :inner].stride(0) == inner + 64 and C.same(mma(wide[:, :inner], K, V, mask), want)


@pytest.mark.parametrize("d,Gn", [(d, Gn) for d in A.D_KVS for Gn in (7, 17)])
def test_dead_rows_get_zeros_and_live_rows_keep_their_bits(d, Gn):
    q, K, V, mask, _ = case(d, 200, "holes", Gn)
    want = mma(q, K, V, mask)
    for name, pattern in S.live_sets(Gn).items():
        live = dev(pattern)
        on = live != 0
        dead_prompts = ~on.view(S.P, Gn).any(dim=1)                   # none of their K / V may be read
        got = mma(nan_rows(q, ~on), nan_rows(K, dead_prompts), nan_rows(V, dead_prompts), mask, live=live)
        assert not torch.isnan(got.float()).any(), name
        assert C.same(got[on], want[on]), (name, "live rows")
        assert C.same(got[~on], torch.zeros_like(got[~on])), (name, "dead rows")


def test_a_captured_call_replays_with_the_eager_bits():
    d, Gn, Sn = 64, 17, 200
    q, K, V, mask, _ = case(d, Sn, "holes", Gn)
    live = dev(S.live_sets(Gn)["alternating"])
    want = mma(q, K, V, mask, live=live)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mma(q, K, V, mask, live=live)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert C.same(out, want)
