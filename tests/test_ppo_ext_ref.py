"""tests/ppo_ext_ref.py against PyTorch in float64: the value-clipped loss and its manual gradient equal torch.autograd on stable-baselines3's literal expression
(values_pred = old + torch.clamp(values - old, -c, c); F.mse_loss(returns, values_pred)), the shared inputs keep every row away from the band's edges and on all
three sides of them, the bounds behave as derived (exactly zero for the value network when no row is inside the band), and the gate rule is SB3's comparison in
float32."""
import numpy as np
import pytest
import torch

import ppo_ext_ref as X
import ppo_ref as R
from test_ppo_ref import SB3, _module

CVF = 0.2
CASES = [(A, batch) for A in (6, 7) for batch in (1, 2, 33)]


def _torch_loss_vf(m, ob, ac, lp, adv, ret, old, clip, cvf, ent_coef, vf_coef, normalize):
    """PPO.train's minibatch loss with clip_range_vf, as stable-baselines3 writes it"""
    if normalize and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    values, logp, ent = m.evaluate_actions(ob, ac)
    ratio = torch.exp(logp - lp)
    pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    values_pred = old + torch.clamp(values - old, -cvf, cvf)
    vf = torch.nn.functional.mse_loss(ret, values_pred)
    loss = pg + vf_coef * vf - ent_coef * ent.mean()
    return loss, [float(s.detach()) for s in (pg, vf, -ent.mean(), ((ratio - 1) - (logp - lp)).mean(), (torch.abs(ratio - 1) > clip).double().mean(), loss)]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A, batch", CASES)
def test_value_clipped_gradient_and_stats_equal_autograd(usim, A, batch, normalize):
    pr = X.make_problem_vf(A, batch, seed=10 * A + batch, rows=batch + 5, index=batch > 16, clip_range_vf=CVF)
    mb = X.minibatch_vf(pr)
    clip, cvf, ent_coef, vf_coef = R.f32(0.2), R.f32(CVF), R.f32(0.01), 0.5
    ref = X.loss_and_grad_vf(pr["p"], *mb, CVF, clip, ent_coef, vf_coef, normalize)
    m = _module(usim, pr["p"], A)
    loss, stats = _torch_loss_vf(m, *(torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in mb), clip, cvf, ent_coef, vf_coef, normalize)
    loss.backward()
    grads = {k: dict(m.named_parameters())[v].grad.numpy() for k, v in SB3.items()}
    want = R.flatten(grads)
    scale = np.abs(want).max()
    assert scale > 0 and np.abs(ref["grad"] - want).max() <= 1e-12 * scale
    for k, v in R.unflatten(ref["grad"], A).items():                     # field by field, relative to the field's own size (an all-zero field must be exactly zero)
        assert np.abs(v - grads[k]).max() <= 1e-12 * np.abs(grads[k]).max(), k
    np.testing.assert_allclose(ref["stats"][:6], stats, rtol=1e-12, atol=1e-15)
    assert ref["stats"][6] == pytest.approx(np.sqrt((want ** 2).sum()), rel=1e-12)
    if not ref["inside"].any():                                           # no row inside the band: the value network receives no gradient at all
        lo, hi = X._vf_segment(A)
        assert not ref["grad"][lo:hi].any() and not want[lo:hi].any()


def test_a_wide_band_is_the_unclipped_loss():
    """clip_range_vf beyond every |V - old|: ppo_ref.loss_and_grad's own numbers, bit for bit (inside the band V itself is used)"""
    pr = X.make_problem_vf(6, 33, seed=3, clip_range_vf=CVF)
    mb = X.minibatch_vf(pr)
    a, b = X.loss_and_grad_vf(pr["p"], *mb, 100.0), R.loss_and_grad(pr["p"], *mb[:5])
    assert a["inside"].all() and np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["stats"], b["stats"])


@pytest.mark.parametrize("A, batch, rows, index", X.CASES)
def test_inputs_stay_away_from_the_band_edges(A, batch, rows, index):
    """the cases of test_gpu_ppo_vf_clip.py, on the reference alone: every row of the minibatch EDGE_MARGIN from a band edge; from 33 rows on, rows below the
    band, inside it and above it, about a third each"""
    pr = X.case_problem(A, batch, rows, index, CVF)
    if index:
        assert len(np.unique(pr["index"])) < batch and pr["rows"] == 3 * batch
    assert pr["old_values"].dtype == np.float32 and pr["old_values"].shape == (pr["rows"],)
    ref = X.loss_and_grad_vf(pr["p"], *X.minibatch_vf(pr), CVF, keep=True)
    assert X.vf_margin(ref) > X.EDGE_MARGIN == 1e-3
    if batch >= 33:
        d = ref["V"] - ref["old_values"]
        below, inside, above = (d < -ref["cvf"]).mean(), ref["inside"].mean(), (d > ref["cvf"]).mean()
        assert min(below, inside, above) > 0.15 and below + inside + above == pytest.approx(1.0)
        assert np.array_equal(ref["inside"], np.abs(d) <= ref["cvf"])
    again = X.case_problem(A, batch, rows, index, CVF)
    assert np.array_equal(again["old_values"], pr["old_values"])          # deterministic


def test_bounds_follow_the_band():
    pr = X.make_problem_vf(6, 33, seed=3, clip_range_vf=CVF)
    mb = X.minibatch_vf(pr)
    ref, e_grad, e_stats = X.grad_bounds_vf(pr["p"], *mb, CVF, 0.2, 0.01, 0.5, True)
    _, e_grad0, e_stats0 = R.grad_bounds(pr["p"], *mb[:5], 0.2, 0.01, 0.5, True)
    lo, hi = X._vf_segment(6)
    assert e_grad.shape == ref["grad"].shape and np.all(e_grad > 0) and np.all(e_stats > 0)
    assert np.array_equal(e_grad[:lo], e_grad0[:lo]) and np.array_equal(e_grad[hi:], e_grad0[hi:])          # the policy network keeps its bound
    assert np.all(e_grad[lo:hi] <= e_grad0[lo:hi]) and e_grad[lo:hi].sum() < e_grad0[lo:hi].sum()            # fewer rows carry an error into the value network
    assert np.array_equal(e_stats[[0, 2, 3, 4]], e_stats0[[0, 2, 3, 4]])
    assert ref["e_dvo"] < X.EDGE_MARGIN                                    # the worst-case error of the kernel's V - old is inside the margin: it decides alike
    # one row outside the band: its bound is the three float32 roundings, far below the forward pass's, and the gradient's is exactly zero
    one = X.make_problem_vf(6, 1, seed=0, clip_range_vf=CVF)
    for seed in range(1, 16):
        if not X.loss_and_grad_vf(one["p"], *X.minibatch_vf(one), CVF)["inside"][0]:
            break
        one = X.make_problem_vf(6, 1, seed=seed, clip_range_vf=CVF)
    ref1, e1, s1 = X.grad_bounds_vf(one["p"], *X.minibatch_vf(one), CVF, 0.2, 0.0, 0.5, True)
    assert not ref1["inside"][0] and not e1[lo:hi].any() and not ref1["grad"][lo:hi].any()
    assert 0 < s1[1] < 8 * R.U * (1.0 + ref1["stats"][1])


def test_gate_rule():
    f = np.float32
    assert X.gate_rule(0.02, 0.0) == 0 and X.gate_rule(1e9, 0.0) == 0    # target_kl 0: off
    assert X.gate_rule(0.0151, 0.01) == 1 and X.gate_rule(0.0149, 0.01) == 0
    t = f(0.01)
    edge = f(1.5) * t                                                     # the float32 product: equal does not trip, one ulp above does
    assert X.gate_rule(edge, t) == 0 and X.gate_rule(np.nextafter(edge, f(1)), t) == 1 and X.gate_rule(np.nextafter(edge, f(0)), t) == 0
    assert X.gate_rule(float("nan"), 0.01) == 0                           # a NaN statistic fails the comparison, as in SB3
