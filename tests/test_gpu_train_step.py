"""The training step calls the library entries its plan names, and no other (train_step.TrainStep.q_entry / .loss_entry).

Counting pass-through wrappers sit on the five entries a step chooses among (tests/train_step_util.py: on the one cached CDLL,
where every Python route looks them up); one p_losses + backward per case.  dim 16, B = 2, 7x12: the smallest plane at which
both a halo wider than the image (16 > 7) and a multi-quad row occur."""
import pytest

from train_step_util import DEV, count_entries, inputs, sched_and_diffusion, step

pytestmark = pytest.mark.gpu

CASES = [("l1", tile, mask, s) for tile in ("off", "xy") for mask in (False, True) for s in (0, 2)]
CASES += [("l2", "xy", True, 2), ("l1_pred_img", "xy", True, 2)]


@pytest.mark.parametrize("lt,tile,mask,s", CASES, ids=lambda v: str(v))
def test_step_calls_the_entries_of_its_plan(golden, monkeypatch, lt, tile, mask, s):
    from sinddm_amd.synth import hash_randn
    from sinddm_amd.train_step import TrainStep
    net, d, _, _ = sched_and_diffusion(golden, 16, loss_type=lt)
    B, H, W = 2, 7, 12
    x_start, x_orig, noise, t = inputs(B, H, W, 900)
    d.train_tile = (True, True) if tile == "xy" else (False, False)
    if mask:
        w = hash_randn((H, W), 901).abs().mul(0.5).clamp(0, 1)               # a soft map with exact zeros
        w[hash_randn((H, W), 902) < -0.4] = 0.0
        assert 0 < int((w == 0).sum()) < w.numel()
        d.train_weights = [w.to(DEV)] * d.n_scales
    plan = TrainStep(d, (B, 3, H, W), s)
    want = {plan.q_entry: 1}
    if plan.loss_entry is not None:
        want[plan.loss_entry] = 1
    assert (plan.loss_entry is None) == (lt != "l1")                          # the torch loss types call no l1 entry at all
    with monkeypatch.context() as m:
        calls = count_entries(m)
        loss, grads = step(net, d, x_start, x_orig, noise, t, s)
    assert calls == want, (calls, want)
    assert loss == loss and loss > 0 and any(bool(g.abs().sum() > 0) for g in grads.values())
