"""CPU-side checks of the processing sampling step (trlx_ppo_sample_proc,
sampling.PPOLogitsProcessors, ppo_sample_step(processors=, prefix=)):

  1  the tests' oracle (ppo_proc_checks.processed) against the committed rows that transformers'
     own processor classes returned, bit for bit, and against those classes live when
     transformers is installed
  2  header, exports and binding: the declaration, the ctypes struct's fields, order and size
  3  the wrapper's refusals that come before any device call"""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
from test_host_cpu import HEADER
import ppo_proc_checks as C

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "sample_processors.npz")
CASES = [(name, kw, n) for name, kw in C.GOLDEN_CASES for n in C.GOLDEN_PREFIX_LENS]
IDS = [f"{name}-n{n}" for name, _, n in CASES]


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. oracle vs transformers
@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) < 100 * 1024
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def inputs():
    return C.golden_inputs()


def test_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(f"{name}/n{n}" for name, _, n in CASES)
    assert all(v.dtype == torch.float32 and tuple(v.shape) == (C.GOLDEN_B, C.GOLDEN_V) for v in golden.values())


@pytest.mark.parametrize("name,kw,n", CASES, ids=IDS)
def test_oracle_equals_the_committed_transformers_rows(golden, inputs, name, kw, n):
    x, prefixes = inputs
    got = C.processed(x, prefixes[n], **C.case_kwargs(kw, n))
    want = golden[f"{name}/n{n}"]
    assert torch.equal(bits(got), bits(want)), (name, n, (got != want).nonzero().tolist())


def test_the_cases_exercise_every_processor(golden, inputs):
    """The fixture is no row of untouched logits: each processor changes some entry at some
    prefix length, n-gram sizes differ, a multi-token bad word fires, both forced tokens fire."""
    x, _ = inputs
    changed = {name: sum(int((golden[f"{name}/n{n}"] != x).sum()) for n in C.GOLDEN_PREFIX_LENS)
               for name, _ in C.GOLDEN_CASES}
    assert all(v > 0 for v in changed.values()), changed
    assert changed["g1"] > changed["g2"] > changed["g3"] > 0
    bad = golden["bad/n9"]
    assert bad[0, 3] == C.NEG and bad[1, 9] == C.NEG and bool((bad[:, 7] == C.NEG).all())
    assert golden["forced-bos/n1"][0].isfinite().nonzero().tolist() == [[5]]
    assert golden["forced-eos/n9"][0].isfinite().nonzero().tolist() == [[1]]
    assert golden["forced-both/n1"][0].isfinite().nonzero().tolist() == [[1]]   # eos wins


@pytest.mark.parametrize("name,kw,n", CASES, ids=IDS)
def test_oracle_equals_transformers_live(inputs, name, kw, n):
    pytest.importorskip("transformers")
    spec = importlib.util.spec_from_file_location("make_golden_sample_processors",
                                                  os.path.join(GOLDEN_DIR, "make_golden_sample_processors.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    x, prefixes = inputs
    want = mk.hf_rows(x, prefixes[n], **kw)
    got = C.processed(x, prefixes[n], **C.case_kwargs(kw, n))
    assert torch.equal(bits(got), bits(want)), (name, n)


def test_forced_decision_of_the_processors_object():
    pr = P.PPOLogitsProcessors(37, "cpu", forced_bos_token_id=5, forced_eos_token_id=1, max_length=7)
    assert [pr.forced(c) for c in (0, 1, 2, 5, 6, 7)] == [-1, 5, -1, -1, 1, -1]
    assert [pr.forced(c) for c in (0, 1, 6)] == [C.forced_id(c, 5, 1, 7) for c in (0, 1, 6)]
    both = P.PPOLogitsProcessors(37, "cpu", forced_bos_token_id=5, forced_eos_token_id=1, max_length=2)
    assert both.forced(1) == 1   # eos wins
    assert not P.PPOLogitsProcessors(37, "cpu").active and pr.active


def test_bad_word_table_is_ragged_and_drops_the_eos_word():
    pr = P.PPOLogitsProcessors(37, "cpu", bad_words_ids=[[7], [2], [3, 9], [1, 2, 3]], eos_token_id=2)
    assert pr.bad_words_ids == [[7], [3, 9], [1, 2, 3]] and pr.n_bad_words == 3
    assert pr.bad_tokens.tolist() == [7, 3, 9, 1, 2, 3] and pr.bad_offsets.tolist() == [0, 1, 3, 6]
    assert pr.bad_tokens.dtype == pr.bad_offsets.dtype == torch.int64


# ------------------------------------------------------------------ 2. header, exports, binding
CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64}


def header_struct():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct TrlxPpoSampleProcArgs\s*\{(.*?)\}\s*TrlxPpoSampleProcArgs\s*;", txt,
                     flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = re.sub(r"\s+", " ", decl).strip()
        if not decl:
            continue
        m = re.fullmatch(r"(.*?)(\w+)", decl)
        ctype, name = m.group(1).strip(), m.group(2)
        fields.append((name, ctypes.c_void_p if ctype.endswith("*") else CTYPES[ctype]))
    return fields


def test_header_declares_and_the_binding_binds_the_entry():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int trlx_ppo_sample_proc\s*\(([^;]*?)\)\s*;", txt, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")] == ["const TrlxPpoSampleProcArgs* a",
                                                                        "void* stream"]
    res, args = _lib.SIGNATURES["trlx_ppo_sample_proc"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.PpoSampleProcArgs), ctypes.c_void_p]
    assert "PPOLogitsProcessors" in P.__all__ and P.PPOLogitsProcessors is P.sampling.PPOLogitsProcessors
    step = inspect.signature(P.ppo_sample_step).parameters
    assert all(step[k].default is None for k in ("processors", "prefix", "prefix_len"))
    ctor = list(inspect.signature(P.PPOLogitsProcessors.__init__).parameters)[1:]
    assert ctor == ["vocab_size", "device", "repetition_penalty", "no_repeat_ngram_size", "bad_words_ids",
                    "forced_bos_token_id", "forced_eos_token_id", "max_length", "eos_token_id"]


def test_ctypes_struct_mirrors_the_header_struct():
    want = header_struct()
    got = list(_lib.PpoSampleProcArgs._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    assert [t for _, t in got] == [t for _, t in want]

    class Mirror(ctypes.Structure):
        _fields_ = want
    assert ctypes.sizeof(_lib.PpoSampleProcArgs) == ctypes.sizeof(Mirror)
    for n, _ in want:
        assert getattr(_lib.PpoSampleProcArgs, n).offset == getattr(Mirror, n).offset, n
    names = [n for n, _ in want]   # the three blocks, in the order the header documents them
    assert names.index("unfinished") < names.index("ref_logits") < names.index("repetition_penalty")


def test_built_library_exports_the_entry():
    lib = _lib.load()
    assert lib.trlx_ppo_sample_proc.argtypes == _lib.SIGNATURES["trlx_ppo_sample_proc"][1]


# ------------------------------------------------------------------ 3. refusals before any device call
def test_wrapper_refusals_need_no_device():
    cpu = torch.zeros(2, 37)
    ok = P.PPOLogitsProcessors(37, "cpu", repetition_penalty=1.2)
    with pytest.raises(ValueError, match="vocab size 41"):
        P.ppo_sample_step(cpu, processors=P.PPOLogitsProcessors(41, "cpu", repetition_penalty=1.2))
    with pytest.raises(ValueError, match="int64"):
        P.ppo_sample_step(cpu, processors=ok, prefix=torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="unit column stride"):
        P.ppo_sample_step(cpu, processors=ok, prefix=torch.zeros(3, 2, dtype=torch.int64).t())
    with pytest.raises(ValueError, match="prefix_len"):
        P.ppo_sample_step(cpu, processors=ok, prefix=torch.zeros(2, 3, dtype=torch.int64), prefix_len=4)
    with pytest.raises(ValueError, match="processors="):
        P.ppo_sample_step(cpu, prefix=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="max_length"):
        P.PPOLogitsProcessors(37, "cpu", forced_eos_token_id=1)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram_size=-1),
               dict(forced_bos_token_id=37), dict(bad_words_ids=[[1], []]), dict(bad_words_ids=[[37]]),
               dict(bad_words_ids=[]), dict(forced_eos_token_id=-1, max_length=4)):
        with pytest.raises(ValueError):
            P.PPOLogitsProcessors(37, "cpu", **kw)


def test_config_builds_one_processors_object_and_refuses_before_any_device_call():
    cfg = P.PPOConfig(gen_kwargs={"forced_eos_token_id": 1})
    with pytest.raises(ValueError, match="max_length"):
        cfg.sample_step(torch.zeros(2, 37), cur_len=0)
    cfg = P.PPOConfig(gen_kwargs={"repetition_penalty": 1.2, "forced_bos_token_id": 5, "eos_token_id": 1,
                                  "bad_words_ids": [[1], [3, 9]], "max_length": 7, "forced_eos_token_id": 1})
    with pytest.raises(ValueError, match="int64"):
        cfg.sample_step(torch.zeros(2, 37), cur_len=0, prefix=torch.zeros(2, 1))
    (pr,) = cfg._processors.values()
    assert (pr.vocab_size, pr.repetition_penalty, pr.bad_words_ids, pr.forced(1), pr.forced(6)) == \
        (37, 1.2, [[3, 9]], 5, 1)
    with pytest.raises(ValueError):
        cfg.sample_step(torch.zeros(2, 37), cur_len=0, prefix=torch.zeros(2, 1))
    assert list(cfg._processors.values()) == [pr]
    assert P.PPOConfig(gen_kwargs={"repetition_penalty": 1.2}) == P.PPOConfig(gen_kwargs={"repetition_penalty": 1.2})
