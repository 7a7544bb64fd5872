"""tests/bc_ref.py against itself: its manual gradient against central differences of its own loss in float64 (parameters drawn from every field, both loss
forms, with and without the value term), the relation between the two forms at the initial log_std, and the shape of its bound.  No GPU, no library."""
import numpy as np
import pytest

import bc_ref as B
import ppo_ref as R

A, ROWS = 6, 37


@pytest.fixture(scope="module")
def problem():
    pr = B.make_problem(A, ROWS, seed=11)
    return {k: np.asarray(v, dtype=np.float64) for k, v in pr["p"].items()}, pr["obs"], pr["act"], pr["value"]


def _loss(theta, obs, act, value, loss, ent, vf):
    return B.loss_and_grad(R.unflatten(theta, A), obs, act, value, loss, ent, vf)["stats"][5]


@pytest.mark.parametrize("loss", [B.NLL, B.MSE])
@pytest.mark.parametrize("valued", [True, False])
def test_gradient_against_central_differences(problem, loss, valued):
    p, obs, act, value = problem
    value = value if valued else None
    ent, vf = 0.03125, 0.5                                                    # (exact in float32: the reference rounds both as the ABI carries them)
    theta = R.flatten(p).astype(np.float64)
    grad = B.loss_and_grad(p, obs, act, value, loss, ent, vf)["grad"]
    rng = np.random.default_rng(5)
    picked = 0
    for name, sl in B.field_slices(A).items():                               # every field: 24 entries of it, or all it has
        idx = np.arange(sl.start, sl.stop)
        idx = idx if len(idx) <= 24 else rng.choice(idx, 24, replace=False)
        for i in idx:
            h = 1e-5
            up, dn = theta.copy(), theta.copy()
            up[i] += h; dn[i] -= h
            fd = (_loss(up, obs, act, value, loss, ent, vf) - _loss(dn, obs, act, value, loss, ent, vf)) / (2 * h)
            assert abs(fd - grad[i]) <= 1e-7 * max(1.0, abs(grad[i])) + 1e-9, (name, i, fd, grad[i])
            picked += 1
        if not valued and name in B.VF_FIELDS:
            assert not grad[sl].any()                                         # no value term: the value network's gradient is zero
        elif not (loss == B.MSE and name == "log_std"):
            assert np.abs(grad[sl]).max() > 0, name
    assert picked >= 250
    if loss == B.MSE:
        assert np.array_equal(grad[-A:], np.full(A, -ent))                    # the policy term does not reach log_std; the entropy term does


def test_nll_gradient_is_the_scaled_mse_gradient_at_the_initial_log_std(problem):
    """log_std = 0 (MlpActorCritic's initial value): d(-log-prob) / d mean = (mean - act) / sigma^2 = d(sum (mean - act)^2) / d mean x 1 / (2 sigma^2)"""
    p, obs, act, _ = problem
    for ls in (0.0, -0.4):                                                    # the initial value, and any other state-independent one
        q = dict(p, log_std=np.full(A, ls))
        nll, mse = (B.loss_and_grad(q, obs, act, None, f, 0.0, 0.5, keep=True) for f in (B.NLL, B.MSE))
        scale = 1.0 / (2.0 * np.exp(2.0 * ls))
        np.testing.assert_allclose(nll["dmean"], scale * mse["dmean"], rtol=1e-13, atol=0)
        sl = B.field_slices(A)
        for name in ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "act_w", "act_b"):
            np.testing.assert_allclose(nll["grad"][sl[name]], scale * mse["grad"][sl[name]], rtol=1e-10, atol=1e-18)
        assert nll["stats"][3] == mse["stats"][3] and nll["stats"][4] == mse["stats"][4]      # action_mse and the mean log-prob do not depend on the form


def test_statistics_are_what_their_names_say(problem):
    p, obs, act, value = problem
    q = B.loss_and_grad(p, obs, act, value, B.NLL, 0.01, 0.25, keep=True)
    s, ent = q["stats"], R.f32(0.01)
    sigma = np.exp(q["ls"])
    logp = (-0.5 * ((act - q["pi"]["out"]) / sigma) ** 2 - q["ls"] - 0.5 * np.log(2 * np.pi)).sum(1)
    assert np.isclose(s[0], -logp.mean(), rtol=1e-13) and np.isclose(s[4], logp.mean(), rtol=1e-13)
    assert np.isclose(s[1], ((value - q["V"]) ** 2).mean(), rtol=1e-13)
    assert np.isclose(s[2], -(q["ls"].sum() + A / 2 * (1 + np.log(2 * np.pi))), rtol=1e-13)
    assert np.isclose(s[3], ((q["pi"]["out"] - act) ** 2).sum(1).mean(), rtol=1e-13)
    assert np.isclose(s[5], s[0] + 0.25 * s[1] + ent * s[2], rtol=1e-13) and np.isclose(s[6], np.linalg.norm(q["grad"]), rtol=1e-13)
    m = B.loss_and_grad(p, obs, act, value, B.MSE, 0.01, 0.0)                 # vf_coef == 0: no value term either
    assert m["stats"][0] == m["stats"][3] and m["stats"][1] == 0.0


@pytest.mark.parametrize("loss", [B.NLL, B.MSE])
def test_bound_is_positive_where_the_gradient_is_computed_and_zero_where_it_is_not(problem, loss):
    p, obs, act, value = problem
    ref, e_grad, e_stats = B.grad_bounds(p, obs, act, None, loss, 1e-3, 0.5)
    sl = B.field_slices(A)
    for name in B.VF_FIELDS:
        assert not e_grad[sl[name]].any() and not ref["grad"][sl[name]].any()
    for name in ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "act_w", "act_b"):
        assert (e_grad[sl[name]] > 0).all()
    assert (e_stats > 0).all() and np.isfinite(e_grad).all()
    # the bound tightens with the rounding unit: nothing in it is a constant floor
    _, e2, _ = B.grad_bounds(p, obs, act, None, loss, 1e-3, 0.5, u={k: v / 4 for k, v in R.UNITS.items()})
    assert (e2[sl["pi_w2"]] < 0.3 * e_grad[sl["pi_w2"]]).all()
    ref_v, e_v, _ = B.grad_bounds(p, obs, act, value, loss, 1e-3, 0.5)
    assert (e_v[sl["vf_w2"]] > 0).all() and np.abs(ref_v["grad"][sl["vf_w2"]]).max() > 0
    # a dropped row would be seen: the largest bound is a small fraction of one row's share of the largest entry (ppo_ref's bound stands at a thirtieth at 33 rows)
    one_row = np.abs(ref_v["grad"]).max() / ROWS
    assert e_v.max() < one_row / 30


def test_clamped_index_list():
    pr = B.make_problem(A, 40, seed=3, rows=90, index=True)
    idx = pr["index"]
    assert (idx < 0).any() and (idx >= 90).any() and len(np.unique(idx)) < len(idx)
    c = B.clamp_index(idx, 90)
    assert c.min() == 0 and c.max() == 89 and np.array_equal(c[(idx >= 0) & (idx < 90)], idx[(idx >= 0) & (idx < 90)])
    obs, act, value = B.minibatch(pr)
    assert obs.shape == (40, 19) and act.shape == (40, A) and value.shape == (40,) and np.abs(act).max() <= 1.0
