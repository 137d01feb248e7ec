"""pipeline_step_from_hidden's submit-time guards: batch k's loss runs inside
call k+1, so
  * a new_hidden / new_weight the loss side cannot take is refused when batch k is SUBMITTED,
    before any launch — the pending batch and the buffers stay as they were, and the next
    good call still returns the earlier batch's results;
  * an in-place update of new_weight between the submitting call and the call running the
    loss (an optimizer.step in between) is refused instead of pairing hidden(k) with W(k+1) —
    new_hidden likewise — at the top of that call (or of pipeline_flush), before anything is
    launched or swapped; pipeline_discard() drops the pending batch and the pipeline goes on.
"""
import pytest
import torch

import trlx_t5_amd as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _batch(B, T, V, H, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, T, H, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(V, H, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    new_h = (h.float() + 0.05 * torch.randn(B, T, H, generator=g).to(DEV)).to(torch.bfloat16)
    labels = torch.randint(0, V, (B, T), generator=g).to(DEV)
    old_values = torch.randn(B, T, generator=g).to(DEV)
    values = old_values + 0.3
    scores = (torch.rand(B, generator=g) * 24 - 12).to(DEV)
    return h, w, new_h, labels, old_values, values, scores


def test_bad_loss_operands_refused_at_submit():
    B, T, V, H = 4, 8, 1031, 512
    h, w, new_h, labels, ov, v, sc = _batch(B, T, V, H, 1)
    hp = P.PPOHotPath(P.PPOConfig(), B, T, V, torch.bfloat16, DEV, kl_coef=0.05)
    assert hp.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc) is None
    pending = hp._pending
    for bad in (new_h.float(), new_h[:, :, :256].contiguous()):
        with pytest.raises(ValueError):
            hp.pipeline_step_from_hidden(h, w, h, w, bad, labels, ov, v, sc)
        assert hp._pending is pending
    with pytest.raises(ValueError):  # a fused loss route at an H it is not built for
        hp.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc,
                                     new_weight=torch.zeros(V, 1024, dtype=torch.bfloat16, device=DEV))
    assert hp._pending is pending
    out = hp.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc)
    torch.cuda.synchronize()
    assert out is not None and torch.isfinite(out[0]).all()
    # the same batch again on a fresh hot path: the refused calls changed nothing
    hp2 = P.PPOHotPath(P.PPOConfig(), B, T, V, torch.bfloat16, DEV, kl_coef=0.05)
    hp2.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc)
    out2 = hp2.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc)
    torch.cuda.synchronize()
    for a, b in zip(out, out2):
        assert torch.equal(a, b)


def test_in_place_weight_update_between_submit_and_loss_refused():
    B, T, V, H = 4, 8, 1031, 512
    h, w, new_h, labels, ov, v, sc = _batch(B, T, V, H, 2)
    hp = P.PPOHotPath(P.PPOConfig(), B, T, V, torch.bfloat16, DEV, kl_coef=0.05)
    wn = w.clone()
    hp.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc, new_weight=wn)
    wn.mul_(1.0)  # an optimizer step in place
    with pytest.raises(RuntimeError, match="modified in place"):
        hp.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc, new_weight=wn)


@pytest.mark.parametrize("edited", ["new_weight", "new_hidden"])
@pytest.mark.parametrize("entry", ["step", "flush"])
def test_in_place_update_refused_before_any_launch_and_recoverable(edited, entry):
    """The refusal comes at the top of the call running the pending loss (the next
    pipeline_step_from_hidden, or pipeline_flush), before batch k+1's experience is launched or
    the lp buffers are swapped: the pending batch and the experience outputs are as they were,
    the refusal repeats while the pending batch stays, and pipeline_discard() is the way out —
    after it the pipeline gives the bits of a fresh hot path."""
    B, T, V, H = 4, 8, 1031, 512
    h, w, new_h, labels, ov, v, sc = _batch(B, T, V, H, 2)
    h2 = (h.float() * 0.5).to(torch.bfloat16)  # batch k+1's experience would overwrite lp_old / ref_lp
    hp = P.PPOHotPath(P.PPOConfig(), B, T, V, torch.bfloat16, DEV, kl_coef=0.05)
    wn, hn = w.clone(), new_h.clone()
    assert hp.pipeline_step_from_hidden(h, w, h, w, hn, labels, ov, v, sc, new_weight=wn) is None
    torch.cuda.synchronize()
    pending, lp_old, ref_lp = hp._pending, hp.lp_old, hp.ref_lp
    before = [t.clone() for t in (lp_old, ref_lp)]
    (wn if edited == "new_weight" else hn).mul_(1.0)  # an optimizer step in place
    for _ in range(2):
        with pytest.raises(RuntimeError, match="modified in place"):
            if entry == "step":
                hp.pipeline_step_from_hidden(h2, w, h2, w, new_h, labels, ov, v, sc, new_weight=w.clone())
            else:
                hp.pipeline_flush()
        torch.cuda.synchronize()
        assert hp._pending is pending
        assert hp.lp_old is lp_old and hp.ref_lp is ref_lp
        for t, b in zip((lp_old, ref_lp), before):
            assert torch.equal(t, b)
    with pytest.raises(RuntimeError, match="pending batch"):  # the serial entry points still refuse
        hp.experience_from_hidden(h, w, h, w, labels, ov, sc)
    assert hp.pipeline_discard() is True
    assert hp._pending is None and hp.pipeline_discard() is False and hp.pipeline_flush() is None
    # recovered: the batch again with an untouched copy of the weight, against a fresh hot path
    assert hp.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc, new_weight=w.clone()) is None
    out = hp.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc, new_weight=w.clone())
    torch.cuda.synchronize()
    hp2 = P.PPOHotPath(P.PPOConfig(), B, T, V, torch.bfloat16, DEV, kl_coef=0.05)
    hp2.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc, new_weight=w.clone())
    out2 = hp2.pipeline_step_from_hidden(h, w, h, w, new_h, labels, ov, v, sc, new_weight=w.clone())
    torch.cuda.synchronize()
    assert out is not None and torch.isfinite(out[0]).all()
    for a, b in zip(out, out2):
        assert torch.equal(a, b)
    assert torch.equal(hp.lp_old, hp2.lp_old) and torch.equal(hp.pipeline_flush()[0], hp2.pipeline_flush()[0])
