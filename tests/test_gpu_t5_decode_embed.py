"""trlx_t5_decode_embed on the GPU (csrc/t5_rmsnorm.hip k_t5_decode_embed; t5_decode.t5_decode_embed):
the decoder's input row of a decode step against F.embedding and t5_rmsnorm.

Every comparison is equality of the raw bits: h is a copy of a table row, and y runs the row tile,
the sum order and the product of k_t5_rmsnorm_fwd.  The table, the tokens and both outputs are
slices of larger allocations with guard margins on both sides, so that even a missing guard in the
kernel would stay inside the test's own memory; the margins are checked afterwards."""
import ctypes

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import t5_rollout_checks as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = (torch.bfloat16, torch.float32)
V, T, LD_TOK, START = 37, 6, 9, 5
# both sides of every form break of kRnBreaks (512, 1024, 2048, 4096, 8192; 1024 is also the one-wave
# limit), and 101: no multiple of the vector width in either dtype, the element form
DS = (64, 96, 101, 512, 520, 1024, 1032, 2048, 4096, 8192)
BS = (1, 3, 5)
_CASES = {}


def case(dtype, D, B):
    """One (dtype, D, B), made once and never modified: the table [V, D] with row stride D + 8 and the
    tokens [B, T] with row stride 9, each inside guard margins (the tokens' guard is a valid id), the
    norm weight."""
    key = (dtype, D, B)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * D + 10 * B + (1 if dtype == torch.float32 else 0))
        ld_w = D + 8
        w_all, weight = C.with_margins((V, D), dtype, DEV, ld_w, ld=ld_w)
        weight.copy_(torch.randn(V, D, generator=g).to(dtype))
        t_all, tokens = C.with_margins((B, T), torch.int64, DEV, LD_TOK, ld=LD_TOK, fill=1)
        tok = torch.randint(0, V, (B, T), generator=g)
        tok[0, 0], tok[-1, 4] = 0, V - 1                    # ids 0 and V - 1 are read at t = 1 and t = 5
        if B > 1:
            tok[1, 0], tok[0, 4] = V - 1, 0
        tokens.copy_(tok)
        norm_w = (1.0 + 0.2 * torch.randn(D, generator=g)).to(dtype).to(DEV)
        _CASES[key] = dict(w_all=w_all, weight=weight, t_all=t_all, tokens=tokens, norm_w=norm_w,
                           w_before=w_all.clone(), t_before=t_all.clone())
    return _CASES[key]


def outputs(B, D, dtype):
    """Guard-filled h and y of row stride D + 8 inside guard margins: (h_all, h, y_all, y)."""
    h_all, h = C.with_margins((B, D), dtype, DEV, D + 8, ld=D + 8)
    y_all, y = C.with_margins((B, D), dtype, DEV, D + 8, ld=D + 8)
    return h_all, h, y_all, y


def margins_kept(whole, view):
    """Everything of `whole` outside `view`'s elements still holds the guard."""
    probe = whole.clone()
    lo = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    rows, cols = view.shape
    probe[lo:lo + rows * view.stride(0)].view(rows, view.stride(0))[:, :cols] = C.GUARD
    return C.same(probe, torch.full_like(probe, C.GUARD))


def set_clock(clock, t):
    clock.record[_lib.CLOCK_T] = t


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("dtype", DTYPES, ids=C.name)
def test_the_row_is_the_table_row_and_its_norm(dtype, D):
    for B in BS:
        c = case(dtype, D, B)
        clock = P.T5DecodeClock(T, DEV)
        for t in (0, 1, 5):
            h_all, h, y_all, y = outputs(B, D, dtype)
            got_h, got_y = P.t5_decode_embed(c["weight"], c["tokens"], t, START, c["norm_w"], out=(h, y))
            assert got_h is h and got_y is y
            want = C.embed_reference(c["weight"], c["tokens"], t, START)
            assert C.same(h, want), (B, t, "h")
            assert C.same(y, P.t5_rmsnorm(h.contiguous(), c["norm_w"])), (B, t, "y")
            assert C.same(y, P.t5_rmsnorm(h, c["norm_w"])), (B, t, "y, rows read in place")
            assert margins_kept(h_all, h) and margins_kept(y_all, y)
            # the clock form is the host form
            set_clock(clock, t)
            ch_all, ch, cy_all, cy = outputs(B, D, dtype)
            P.t5_decode_embed(c["weight"], c["tokens"], clock, START, c["norm_w"], out=(ch, cy))
            assert C.same(ch, h) and C.same(cy, y), (B, t, "clock")
            assert margins_kept(ch_all, ch) and margins_kept(cy_all, cy) and clock.t == t
            # without norm_weight: y is None, h as before
            h2, y2 = P.t5_decode_embed(c["weight"], c["tokens"], t, START)
            assert y2 is None and C.same(h2, h)
            set_clock(clock, t)
            h3, y3 = P.t5_decode_embed(c["weight"], c["tokens"], clock, START)
            assert y3 is None and C.same(h3, h)
        assert C.same(c["w_all"], c["w_before"]) and C.same(c["t_all"], c["t_before"])


def test_t_zero_is_the_start_token_and_t_equal_T_reads_the_last_column():
    c = case(torch.bfloat16, 96, 3)
    h, _ = P.t5_decode_embed(c["weight"], c["tokens"], 0, START)
    assert C.same(h, c["weight"][START].expand(3, 96))
    h, _ = P.t5_decode_embed(c["weight"], c["tokens"], T, START)
    assert C.same(h, c["weight"][c["tokens"][:, T - 1]])
    clock = P.T5DecodeClock(T + 4, DEV)                    # a clock that outlasts the tokens: t = T is still live
    set_clock(clock, T)
    hc, _ = P.t5_decode_embed(c["weight"], c["tokens"], clock, START)
    assert C.same(hc, h)
    rec = P.PPORolloutRecorder(3, T, DEV, pad_token_id=0, eos_token_id=1)
    rec.tokens.copy_(c["tokens"])
    assert C.same(P.t5_decode_embed(c["weight"], rec, 2, START)[0], c["weight"][c["tokens"][:, 1]])


@pytest.mark.parametrize("cap,t", [(T, -1), (T, T), (T + 4, T + 1), (T + 4, T + 3), (T + 4, T + 4), (T + 4, T + 7),
                                   (T, 1 << 40)], ids=str)
@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 96), (torch.float32, 1032), (torch.bfloat16, 101)], ids=str)
def test_a_dead_step_writes_zeros_and_reads_nothing(dtype, D, cap, t):
    assert not (0 <= t < cap and t - 1 < T)
    B = 3
    c = case(dtype, D, B)
    # NaN in the table and a negative norm weight: a dead step that read either would not give +0
    w_all, weight = C.with_margins((V, D), dtype, DEV, D + 8, ld=D + 8, fill=float("nan"))
    norm_w = -torch.ones(D, dtype=dtype, device=DEV)
    clock = P.T5DecodeClock(cap, DEV)
    set_clock(clock, t)
    h_all, h, y_all, y = outputs(B, D, dtype)
    P.t5_decode_embed(weight, c["tokens"], clock, START, norm_w, out=(h, y))
    torch.cuda.synchronize()
    assert C.same(h, torch.zeros(B, D, dtype=dtype, device=DEV)) and C.same(y, torch.zeros(B, D, dtype=dtype, device=DEV))
    assert margins_kept(h_all, h) and margins_kept(y_all, y) and C.same(c["t_all"], c["t_before"])
    assert clock.record.tolist() == [t, cap, 1, 0, 0, 0, 0, 0]
    h2_all, h2 = C.with_margins((B, D), dtype, DEV, D + 8, ld=D + 8)
    P.t5_decode_embed(weight, c["tokens"], clock, START, out=(h2, None))
    assert C.same(h2, torch.zeros(B, D, dtype=dtype, device=DEV)) and margins_kept(h2_all, h2)


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 96), (torch.float32, 2048), (torch.float32, 101)], ids=str)
def test_ids_outside_the_table_give_zero_rows(dtype, D):
    B = 5
    c = case(dtype, D, B)
    tokens = c["tokens"].clone()
    tokens[:, 2] = torch.tensor([-1, V, 3, -(1 << 40), 1 << 40], device=DEV)
    h_all, h, y_all, y = outputs(B, D, dtype)
    P.t5_decode_embed(c["weight"], tokens, 3, START, c["norm_w"], out=(h, y))
    want = C.embed_reference(c["weight"], tokens, 3, START)
    assert C.same(h, want) and not h[0].any() and not h[1].any() and not h[3].any() and not h[4].any() and h[2].any()
    assert C.same(y, P.t5_rmsnorm(h, c["norm_w"]))
    assert margins_kept(h_all, h) and margins_kept(y_all, y) and C.same(c["w_all"], c["w_before"])
    for start in (-1, V):                                        # the start token is tested the same way
        h0, _ = P.t5_decode_embed(c["weight"], tokens, 0, start)
        assert not h0.any()


def test_out_is_written_in_place_and_a_second_call_allocates_nothing():
    c = case(torch.bfloat16, 512, 5)
    clock = P.T5DecodeClock(T, DEV)
    h = torch.full((5, 512), C.GUARD, dtype=torch.bfloat16, device=DEV)
    y = torch.full_like(h, C.GUARD)
    for t in (2, clock):
        P.t5_decode_embed(c["weight"], c["tokens"], t, START, c["norm_w"], out=(h, y))
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        got = P.t5_decode_embed(c["weight"], c["tokens"], t, START, c["norm_w"], out=(h, y))
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        assert got[0] is h and got[1] is y
    set_clock(clock, 2)
    P.t5_decode_embed(c["weight"], c["tokens"], clock, START, c["norm_w"], out=(h, y))
    assert C.same(h, c["weight"][c["tokens"][:, 1]]) and C.same(y, P.t5_rmsnorm(h, c["norm_w"]))


def test_refusals_launch_nothing():
    dtype, D, B = torch.bfloat16, 96, 3
    c = case(dtype, D, B)
    h_all, h, y_all, y = outputs(B, D, dtype)
    clock = P.T5DecodeClock(T, DEV)
    stream = _lib.stream_of(h)
    esz = 2

    def embed(clock_ptr=None, **over):
        a = _lib.T5DecodeEmbedArgs(
            weight=c["weight"].data_ptr(), ld_w=D + 8, tokens=c["tokens"].data_ptr(), ld_tokens=LD_TOK,
            norm_w=c["norm_w"].data_ptr(), h=h.data_ptr(), ld_h=D + 8, y=y.data_ptr(), ld_y=D + 8, B=B, D=D, V=V, T=T, t=1,
            start_token_id=START, eps=1e-6, dtype=_lib.BF16)
        for k, v in over.items():
            setattr(a, k, v)
        return _lib.query("trlx_t5_decode_embed", ctypes.byref(a), clock_ptr, stream)

    rec = clock.record.data_ptr()
    arg = [dict(weight=None), dict(tokens=None), dict(h=None), dict(y=None), dict(norm_w=None),
           dict(weight=c["weight"].data_ptr() + 1), dict(h=h.data_ptr() + 1), dict(y=y.data_ptr() + 1),
           dict(norm_w=c["norm_w"].data_ptr() + 1), dict(tokens=c["tokens"].data_ptr() + 4), dict(t=-1), dict(t=T + 1),
           # a written operand over any other operand
           dict(y=h.data_ptr()), dict(y=h.data_ptr() + (D + 8) * esz), dict(h=c["weight"].data_ptr() + 5 * (D + 8) * esz),
           dict(y=c["norm_w"].data_ptr()), dict(h=c["tokens"].data_ptr()), dict(eps=float("nan"))]
    for over in arg:
        assert embed(**over) == C.ERR_ARG, over
    assert embed(rec + 4) == C.ERR_ARG
    assert embed(rec, h=rec, ld_h=D, B=1, y=None, norm_w=None, D=16) == C.ERR_ARG      # h over the clock
    assert _lib.query("trlx_t5_decode_embed", None, None, stream) == C.ERR_ARG
    for over in (dict(D=0), dict(D=8193), dict(B=0), dict(V=0), dict(T=0)):
        assert embed(**over) == C.ERR_SHAPE, over
    for over in (dict(ld_w=D - 1), dict(ld_h=D - 1), dict(ld_y=D - 1), dict(ld_tokens=T - 1)):
        assert embed(**over) == C.ERR_STRIDE, over
    for over in (dict(dtype=_lib.I64), dict(dtype=7)):
        assert embed(**over) == C.ERR_DTYPE, over
    torch.cuda.synchronize()
    for whole in (h_all, y_all):
        assert C.same(whole, torch.full_like(whole, C.GUARD))
    assert C.same(c["w_all"], c["w_before"]) and C.same(c["t_all"], c["t_before"])
    assert embed() == 0 and embed(rec, t=T + 9) == 0             # the call they were built from runs; a->t unread
    torch.cuda.synchronize()
    assert C.same(h, c["weight"][START].expand(B, D))            # the clock stands at 0
    # the wrapper's own refusals
    with pytest.raises(ValueError):
        P.t5_decode_embed(c["weight"], c["tokens"], T + 1, START)
    with pytest.raises(ValueError):
        P.t5_decode_embed(c["weight"], c["tokens"].cpu(), 0, START)
    with pytest.raises(ValueError):
        P.t5_decode_embed(c["weight"], c["tokens"], P.T5DecodeClock(T, "cpu"), START)
    with pytest.raises(ValueError):
        P.t5_decode_embed(c["weight"], c["tokens"], 0, START, c["norm_w"], out=(h, None))
