"""The decode clock without a GPU: the header's declarations, the ctypes mirror, the binding's symbol
list, the clock's rule against PPOLogitsProcessors.forced, and the argument refusals that need no
device."""
import ctypes
import itertools
import os
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
import decode_clock_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "trlx_t5_amd.h")).read()


def test_the_header_declares_the_clock_entries_and_keeps_the_abi_version():
    flat = re.sub(r"\s+", " ", HEADER)
    for decl in ("int trlx_decode_clock_init(int64_t* clock, int64_t T, int64_t cur_len0, void* stream);",
                 "int trlx_decode_clock_advance(int64_t* clock, void* stream);",
                 "int trlx_t5_decode_attn_dev(const TrlxT5DecodeAttnArgs* a, const int64_t* clock, void* stream);",
                 "int trlx_ppo_sample_proc_dev(const TrlxPpoSampleProcArgs* a, const TrlxPpoSampleDevArgs* d, "
                 "void* stream);",
                 "} TrlxPpoSampleDevArgs;"):
        assert decl in flat, decl
    assert re.search(r"#define TRLX_ABI_VERSION 2\b", HEADER) and _lib.ABI_VERSION == 2
    for name, word in (("T", 0), ("CAP", 1), ("CUR_LEN0", 2), ("OVERRUN", 3), ("WORDS", 8)):
        assert re.search(rf"#define TRLX_CLOCK_{name} {word}\b", HEADER)
    assert (_lib.CLOCK_T, _lib.CLOCK_CAP, _lib.CLOCK_CUR_LEN0, _lib.CLOCK_OVERRUN, _lib.CLOCK_WORDS) == (0, 1, 2, 3, 8)
    assert C.CLOCK_WORDS == _lib.CLOCK_WORDS


def test_the_ctypes_mirror_has_the_headers_field_order_and_size():
    body = re.search(r"typedef struct TrlxPpoSampleDevArgs \{(.*?)\} TrlxPpoSampleDevArgs;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.match(r"(.*?)(\w+)$", f.strip()).groups() for f in body.split(";") if f.strip()]
    assert [n for _, n in fields] == [n for n, _ in _lib.PpoSampleDevArgs._fields_]
    assert [n for _, n in fields] == ["clock", "forced_bos_token_id", "forced_eos_token_id", "max_length", "u_ld"]
    for (ctype, name), (_, py) in zip(fields, _lib.PpoSampleDevArgs._fields_):
        assert py is (ctypes.c_void_p if "*" in ctype else ctypes.c_int64), (ctype, name)
    assert ctypes.sizeof(_lib.PpoSampleDevArgs) == 40


def test_the_binding_lists_the_new_symbols():
    sig = _lib.SIGNATURES
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert sig["trlx_decode_clock_init"] == (ctypes.c_int, [vp, i64, i64, vp])
    assert sig["trlx_decode_clock_advance"] == (ctypes.c_int, [vp, vp])
    assert sig["trlx_t5_decode_attn_dev"] == (ctypes.c_int, [ctypes.POINTER(_lib.T5DecodeAttnArgs), vp, vp])
    assert sig["trlx_ppo_sample_proc_dev"] == (ctypes.c_int, [ctypes.POINTER(_lib.PpoSampleProcArgs),
                                                              ctypes.POINTER(_lib.PpoSampleDevArgs), vp])
    assert "T5DecodeClock" in P.__all__ and P.T5DecodeClock is P.t5_decode.T5DecodeClock


@pytest.mark.parametrize("max_length", (2, 3, 7))
@pytest.mark.parametrize("use_bos,use_eos", list(itertools.product((False, True), repeat=2)))
def test_the_clock_rule_is_the_processors_forced_rule(use_bos, use_eos, max_length):
    """For every cur_len in [0, max_length + 2] (cur_len0 0 and 1, every t that gives it): the forced
    token of the rule is PPOLogitsProcessors.forced(cur_len); max_length 2 is the step where bos
    and eos both fire and eos wins; the eos suppression is cur_len < min_length."""
    V, bos, feos, eos, min_length = 11, 4, 9, 2, 3
    procs = P.PPOLogitsProcessors(V, "cpu", forced_bos_token_id=bos if use_bos else None,
                                  forced_eos_token_id=feos if use_eos else None, max_length=max_length)
    T = max_length + 3
    seen = set()
    for cur_len0 in (0, 1):
        for t in range(-1, T + 2):
            r = C.clock_rule(t, T, cur_len0, min_length=min_length, eos=eos, forced_bos=bos if use_bos else -1,
                             forced_eos=feos if use_eos else -1, max_length=max_length)
            assert r["live"] == (0 <= t < T)
            if not r["live"]:
                continue
            assert r["cur_len"] == cur_len0 + t
            assert r["forced"] == procs.forced(r["cur_len"])
            assert r["suppress_eos"] == (r["cur_len"] < min_length)
            seen.add(r["cur_len"])
    assert seen >= set(range(0, max_length + 3))
    if use_bos and use_eos and max_length == 2:
        assert C.clock_rule(0, T, 1, forced_bos=bos, forced_eos=feos, max_length=2)["forced"] == feos
    # a shorter record buffer bounds the live steps too; no eos given: nothing to suppress
    assert not C.clock_rule(3, T, 1, buffers_T=3)["live"] and C.clock_rule(2, T, 1, buffers_T=3)["live"]
    assert not C.clock_rule(0, T, 0, min_length=5)["suppress_eos"]


def test_the_attention_geometry_and_the_sampler_table_are_the_kernels():
    assert [C.groups(dt, d) for dt in (torch.bfloat16, torch.float32) for d in (64, 128)] == [32, 16, 16, 8]
    assert C.self_t(torch.float32, 128, 70) == [0, 1, 7, 8, 15, 16, 17, 69]
    src = open(os.path.join(ROOT, "trlx-t5_amd", "csrc", "ppo_sample.hip")).read()
    for dt, name in ((torch.bfloat16, "BF16T"), (torch.float32, "F32T")):
        rows = [(int(n), int(nt)) for n, nt in re.findall(rf"TRLX_PSMP\({name}, (\d+), (\d+)\)", src)]
        assert tuple(rows) == C.SAMPLER_BRANCHES[dt]
        vs = C.sampler_vocabs(dt)
        assert all(C.sampler_branch(v, dt) == b for b, v in vs) and vs[0] == (0, 517)
        assert all(C.sampler_branch(v - 1, dt) < b for b, v in vs[1:])
        # every row of the table that any V can reach is in the list
        reachable = {C.sampler_branch(v, dt) for v in range(1, 60000, 7)} - {None}
        assert reachable == {b for b, _ in vs}, (reachable, vs)
    assert f"kLineVecs = {C.LINE_VECS};" in open(os.path.join(ROOT, "trlx-t5_amd", "csrc", "common.h")).read()


def test_refusals_that_need_no_device():
    with pytest.raises(ValueError):
        P.T5DecodeClock(0, "cpu")
    with pytest.raises(ValueError):
        P.T5DecodeClock(4, "cpu", cur_len0=-1)
    clock = P.T5DecodeClock(4, "cpu")
    assert clock.record.tolist() == [0, 4, 1, 0, 0, 0, 0, 0] and clock.t == 0 and clock.overrun == 0
    with pytest.raises(ValueError, match="capacity"):
        P.PPORolloutRecorder(2, 5, "cpu", pad_token_id=0, eos_token_id=1, clock=clock)
    with pytest.raises(ValueError):
        P.PPORolloutRecorder(2, 4, "cpu", pad_token_id=0, eos_token_id=1, clock=object())
    rec = P.PPORolloutRecorder(2, 4, "cpu", pad_token_id=0, eos_token_id=1, clock=clock)
    clock.record[0] = 9
    assert rec.sync_t() == 4      # min(clock.t, T)
    rec.reset()
    assert clock.record.tolist() == [0, 4, 1, 0, 0, 0, 0, 0] and rec.t == 0
    logits = torch.zeros(2, 13)
    with pytest.raises(ValueError, match="cur_len"):
        P.ppo_sample_step(logits, ref_logits=logits, recorder=rec, cur_len=1)
    for u in (torch.zeros(4, 3), torch.zeros(3, 2), torch.zeros(4, 2, dtype=torch.float64), torch.zeros(2, 4).t()):
        with pytest.raises(ValueError, match="u table"):
            P.ppo_sample_step(logits, ref_logits=logits, recorder=rec, u=u)
    # a clock in place of t: the capacity must fit the cache, and a shape the kernel does not take is refused
    cache = P.T5DecodeKVCache(1, 1, 64, 3, torch.float32, "cpu")
    q = torch.zeros(1, 64)
    with pytest.raises(ValueError, match="max_len"):
        P.t5_decode_self_attention(q, q, q, cache, clock)
    cache = P.T5DecodeKVCache(1, 1, 32, 8, torch.float32, "cpu")
    with pytest.raises(ValueError, match="captured"):
        P.t5_decode_self_attention(q[:, :32], q[:, :32], q[:, :32], cache, clock)
