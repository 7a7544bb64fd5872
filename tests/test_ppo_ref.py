"""tests/ppo_ref.py against PyTorch in float64: the manual backward pass equals torch.autograd on policy.MlpActorCritic(...).double() with the loss of
tools/ppo_demo.py, clip + Adam equals clip_grad_norm_ + torch.optim.Adam, and the shared test inputs keep every sample away from the kinks of the loss -- so the
GPU tests (test_gpu_ppo_kernels.py) compare the kernels with a reference that is itself checked, and need no exclusion list."""
import numpy as np
import pytest
import torch

import ppo_ref as R

SB3 = {"pi_w1": "policy_net.0.weight", "pi_b1": "policy_net.0.bias", "pi_w2": "policy_net.2.weight", "pi_b2": "policy_net.2.bias", "act_w": "action_net.weight",
       "act_b": "action_net.bias", "vf_w1": "value_net_body.0.weight", "vf_b1": "value_net_body.0.bias", "vf_w2": "value_net_body.2.weight",
       "vf_b2": "value_net_body.2.bias", "val_w": "value_net.weight", "val_b": "value_net.bias", "log_std": "log_std"}


def _module(usim, p, A):
    m = usim.policy.MlpActorCritic(19, A).double()
    m.load_state_dict({SB3[k]: torch.as_tensor(np.asarray(v, dtype=np.float64)) for k, v in p.items()})
    return m


def _torch_loss(m, ob, ac, lp, adv, ret, clip, ent_coef, vf_coef, normalize):
    """the minibatch step of tools/ppo_demo.py, with its constants as arguments"""
    if normalize and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    values, logp, ent = m.evaluate_actions(ob, ac)
    ratio = torch.exp(logp - lp)
    pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vf = torch.nn.functional.mse_loss(values, ret)
    loss = pg + vf_coef * vf - ent_coef * ent.mean()
    stats = [pg, vf, -ent.mean(), ((ratio - 1) - (logp - lp)).mean(), (torch.abs(ratio - 1) > clip).double().mean(), loss]
    return loss, [float(s.detach()) for s in stats]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A, batch, ent_coef", [(6, 97, 0.0), (7, 64, 0.01), (6, 1, 0.01), (7, 2, 0.0)])
def test_gradient_and_stats_equal_autograd(usim, A, batch, ent_coef, normalize):
    pr = R.make_problem(A, batch, seed=10 * A + batch, rows=batch + 5, index=batch > 16)
    mb = R.minibatch(pr)
    clip, vf_coef = R.f32(0.2), 0.5
    ref = R.loss_and_grad(pr["p"], *mb, clip, ent_coef, vf_coef, normalize)
    m = _module(usim, pr["p"], A)
    loss, stats = _torch_loss(m, *(torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in mb), clip, R.f32(ent_coef), vf_coef, normalize)
    loss.backward()
    grads = {k: dict(m.named_parameters())[v].grad.numpy() for k, v in SB3.items()}
    want = R.flatten(grads)
    scale = np.abs(want).max()
    assert scale > 0 and np.abs(ref["grad"] - want).max() <= 1e-10 * scale
    for k, v in R.unflatten(ref["grad"], A).items():                     # ... and field by field, relative to the field's own size
        assert np.abs(v - grads[k]).max() <= 1e-10 * max(np.abs(grads[k]).max(), 1e-300), k
    np.testing.assert_allclose(ref["stats"][:6], stats, rtol=1e-10, atol=1e-14)
    assert ref["stats"][6] == pytest.approx(np.sqrt((want ** 2).sum()), rel=1e-10)


def test_flat_order_is_the_header_order():
    for A in (6, 7):
        p = R.make_params(A, 0)
        assert R.flatten(p).size == R.n_params(A) == 76032 + 130 * A + 129
        back = R.unflatten(R.flatten(p), A)
        assert list(back) == list(R.FIELDS) and all(np.array_equal(back[k], p[k]) for k in p)


def test_adam_equals_torch(usim):
    rng = np.random.default_rng(5)
    n = 1000
    theta, m, v = rng.normal(0, 1, n), np.zeros(n), np.zeros(n)
    lr, eps, mx = R.f32(3e-4), R.f32(1e-5), 0.5
    t = torch.nn.Parameter(torch.as_tensor(theta.copy()))
    opt = torch.optim.Adam([t], lr=lr, betas=(R.f32(0.9), R.f32(0.999)), eps=eps)
    step = 0
    for k in range(5):
        g = rng.normal(0, 0.002 if k % 2 else 0.1, n)                     # the clip is active at every other step
        t.grad = torch.as_tensor(g.copy())
        used = float(torch.nn.utils.clip_grad_norm_([t], mx))
        opt.step()
        theta, m, v, step, norm = R.adam(theta, g, m, v, step, lr, 0.9, 0.999, eps, mx)
        assert norm == pytest.approx(used, rel=1e-12) and (norm > mx) == (k % 2 == 0)
        np.testing.assert_allclose(theta, t.detach().numpy(), rtol=1e-12, atol=1e-15)
        st = opt.state[t]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)
    assert step == 5
    same = R.adam(theta, g, m, v, step, lr, 0.9, 0.999, eps, 0.0)         # max_grad_norm <= 0: no clipping
    big = R.adam(theta, g, m, v, step, lr, 0.9, 0.999, eps, 1e9)
    assert np.array_equal(same[0], big[0])


@pytest.mark.parametrize("A", [6, 7])
@pytest.mark.parametrize("batch, rows, index", [(1, None, False), (2, None, False), (31, None, False), (32, None, False), (33, None, False),
                                                (32 * R.W + 5, None, False), (32 * (R.W + 3) + 7, 3 * (32 * (R.W + 3) + 7), True)])
def test_inputs_stay_away_from_the_kinks(A, batch, rows, index):
    """the cases of test_gpu_ppo_kernels.py: no ratio within 1e-3 of a clip edge, no |advantage| (as the loss uses it) below 1e-3; from 31 samples on, ratios on
    both sides of both edges and advantages of both signs"""
    pr = R.make_problem(A, batch, seed=batch + A, rows=rows, index=index)
    if index:
        assert len(np.unique(pr["index"])) < batch and pr["index"].max() < pr["rows"] == 3 * batch
    for normalize in (False, True):
        ref = R.loss_and_grad(pr["p"], *R.minibatch(pr), 0.2, 0.0, 0.5, normalize)
        edge, small = R.margins(ref)
        assert edge > 1e-3 and small > 1e-3
        if batch >= 31:
            r, ad = ref["ratio"], ref["adv"]
            assert (r < 0.8).any() and ((r > 0.8) & (r < 1.2)).any() and (r > 1.2).any() and (ad > 0).any() and (ad < 0).any()
            passes = ~(((ad > 0) & (r > 1.2)) | ((ad < 0) & (r < 0.8)))
            assert passes.any() and (~passes).any()


def test_bounds_are_positive_and_small(usim):
    """grad_bounds on a small case: a bound for every entry, far below the gradient's own size (the GPU tests compare against it)"""
    pr = R.make_problem(6, 33, seed=3)
    ref, e_grad, e_stats = R.grad_bounds(pr["p"], *R.minibatch(pr), 0.2, 0.01, 0.5, True)
    assert e_grad.shape == ref["grad"].shape and np.all(e_grad > 0) and np.all(e_stats > 0)
    assert e_grad.max() < 2e-3 * np.abs(ref["grad"]).max() and np.all(e_stats[:6] < 1e-3)
    print("largest bound / largest entry", e_grad.max() / np.abs(ref["grad"]).max(), "statistics", e_stats)
