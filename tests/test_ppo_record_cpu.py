"""CPU-side checks of the recording sampling step's surface: the names are exported, the
binding and the header agree on the new entry, and the argument checks that need no device
refuse before touching the library."""
import inspect
import re

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib
from test_host_cpu import HEADER


def test_new_names_are_exported():
    assert "PPORolloutRecorder" in P.__all__ and P.PPORolloutRecorder is P.rollout_store.PPORolloutRecorder
    assert "trlx_ppo_sample_record" in _lib.SIGNATURES
    assert callable(P.PPOHotPath.experience_from_logprobs)
    step = inspect.signature(P.ppo_sample_step).parameters
    assert all(k in step and step[k].default in (None, False)
               for k in ("ref_logits", "recorder", "values", "score_finished"))
    hot = inspect.signature(P.PPOHotPath.experience_from_logprobs).parameters
    assert list(hot)[1:] == ["labels", "old_values", "scores", "logprobs", "ref_logprobs", "lengths", "mask", "group"]
    assert {"reset", "push_to"} <= set(dir(P.PPORolloutRecorder))


def test_header_and_binding_agree_on_the_record_entry():
    """The declaration's parameter count equals the binding's, and it extends trlx_ppo_sample's
    list (the plain entry keeps its own arguments)."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {n: a for n, a in re.findall(r"int (trlx_ppo_sample(?:_record)?)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    args = {n: [re.sub(r"\s+", " ", x).strip() for x in a.split(",")] for n, a in decl.items()}
    assert len(args["trlx_ppo_sample"]) == len(_lib.SIGNATURES["trlx_ppo_sample"][1]) == 20
    assert len(args["trlx_ppo_sample_record"]) == len(_lib.SIGNATURES["trlx_ppo_sample_record"][1])
    assert args["trlx_ppo_sample_record"][:19] == args["trlx_ppo_sample"][:19]
    assert args["trlx_ppo_sample_record"][-1] == "void* stream"
    assert _lib.SIGNATURES["trlx_ppo_sample_record"][1][:19] == _lib.SIGNATURES["trlx_ppo_sample"][1][:19]


def test_recording_keywords_go_together_and_need_a_device():
    cpu = torch.zeros(2, 8)
    with pytest.raises(ValueError):  # no CPU path
        P.ppo_sample_step(cpu, ref_logits=cpu, recorder=object())
