"""imitation.NativeBC on the device, on fixed seeded data (no environment): three minibatch steps against tests/bc_ref.py and ppo_ref.adam, a seed fixes the
result of train(), and ppo.NativePPO built afterwards on the same policy trains the same words.

The bound pattern of the three steps: every step is compared on its own, from the state the device is in before it.  The parameters, Adam's moments and the
gradient are float32 words, read back exactly; the reference gradient is taken at the device's parameters (bound: bc_ref.grad_bounds), and the reference Adam
step is taken from the device's own gradient and moments (bound: ppo_ref.adam_bounds -- the half-ulp of the one rounding of a float64 result).  No error is
carried from one step into the next, so no amplification factor through Adam's division has to be assumed."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bc_ref as B
import ppo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A, ROWS = 6, 300


def _policy(usim, seed):
    torch.manual_seed(seed)
    policy = usim.policy.MlpActorCritic(19, A).to(DEV)
    for m in policy.modules():                                             # SB3's initialisation, as tools/ppo_demo.py
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.orthogonal_(m.weight, gain=2 ** 0.5); torch.nn.init.zeros_(m.bias)
    torch.nn.init.orthogonal_(policy.action_net.weight, gain=0.01); torch.nn.init.orthogonal_(policy.value_net.weight, gain=1.0)
    return policy


def _learner(usim, seed=0, valued=True, **kw):
    pr = B.make_problem(A, ROWS, seed=21)
    demos = usim.DemoBuffer(ROWS + 50, A, DEV)
    t = lambda k: torch.as_tensor(pr[k]).to(DEV)
    demos.add(t("obs"), t("act"), t("value") if valued else None)
    vn = usim.policy.DeviceVecNormalize(1, 19, device=DEV, training=True)  # identity statistics; train() must leave them alone although training is set
    return pr, usim.NativeBC(_policy(usim, seed), vn, demos, seed=seed, **kw)


def _check(name, got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound), f"{name}: worst error / bound {worst:.3g}"
    return worst


@pytest.mark.parametrize("loss, valued", [("nll", True), ("mse", False)])
def test_three_minibatch_steps_against_the_references(usim, loss, valued):
    pr, bc = _learner(usim, seed=4, valued=valued, loss=loss, learning_rate=1e-3)
    d = bc.demos
    obs_n = bc.vecnorm.normalize_obs(d.obs[:ROWS], update=False).contiguous()
    data = (obs_n, d.act[:ROWS]) + ((d.value[:ROWS],) if valued else ())
    perm = np.random.default_rng(9).permutation(ROWS).astype(np.int32)
    x, act, value = obs_n.cpu().numpy(), pr["act"], pr["value"]
    cpu = lambda t: t.detach().cpu().numpy().copy()
    for k, (lo, hi) in enumerate(((0, 100), (100, 233), (233, 300))):       # 100, 133 and 67 rows: more than one tile, none a multiple of it
        idx = perm[lo:hi]
        theta0, m0, v0 = cpu(bc.theta), cpu(bc.exp_avg), cpu(bc.exp_avg_sq)
        bc.minibatch_step(data, torch.as_tensor(idx).to(DEV), hi - lo)
        torch.cuda.synchronize()
        grad, stats = cpu(bc.grad), cpu(bc.stats)
        ref, e_grad, e_stats = B.grad_bounds(R.unflatten(theta0, A), x[idx], act[idx], value[idx] if valued else None, usim.imitation.LOSSES[loss], bc.ent_coef,
                                             bc.vf_coef)
        _check(f"step {k} gradient", grad, ref["grad"], e_grad)
        _check(f"step {k} statistics", stats[:6], ref["stats"][:6], e_stats[:6])
        rt, rm, rv, rs, rnorm = R.adam(theta0, grad, m0, v0, k, 1e-3, 0.9, 0.999, bc.adam_eps, bc.max_grad_norm)
        et, em, ev, en = R.adam_bounds(theta0, rt, rm, rv, rnorm)
        _check(f"step {k} theta", cpu(bc.theta), rt, et); _check(f"step {k} m", cpu(bc.exp_avg), rm, em); _check(f"step {k} v", cpu(bc.exp_avg_sq), rv, ev)
        _check(f"step {k} norm", stats[6], rnorm, en)
        assert int(bc.step_count.item()) == rs == k + 1 and np.abs(cpu(bc.theta) - theta0).max() > 0
        if not valued:
            sl = B.field_slices(A)
            vf = slice(sl["vf_w1"].start, sl["val_b"].stop)
            assert not grad[vf].view(np.uint32).any() and np.array_equal(cpu(bc.theta)[vf], theta0[vf])      # zero gradient, zero moments: the critic stays put
    assert usim.ppo._is_flat(bc.policy, bc.theta)
    assert float(bc.vecnorm._obs_count) == 1e-4 and not bc.vecnorm.obs_mean.any()       # the statistics were read, never updated


def test_train_result_history_and_the_trailing_minibatch(usim):
    _, bc = _learner(usim, seed=1, n_epochs=2, batch_size=128)              # 300 = 128 + 128 + 44
    calls, step = [], bc.minibatch_step
    bc.minibatch_step = lambda data, index, batch, lr=None: (calls.append((int(batch), int(index.numel()), len(data))), step(data, index, batch, lr))[1]
    out = bc.train()
    assert calls == [(128, 128, 3), (128, 128, 3), (44, 44, 3)] * 2 and int(bc.step_count.item()) == 6
    assert tuple(out) == usim.imitation.STAT_NAMES and out["bc/optimizer_steps"] == 6 and bc.history == [out]
    assert all(np.isfinite(v) for v in out.values()) and out["bc/action_mse"] > 0 and out["bc/value_loss"] > 0 and out["bc/entropy_loss"] < 0
    assert tuple(bc.first_minibatch) == usim.imitation.STAT_NAMES and bc.first_minibatch["bc/action_mse"] > 0
    _, full = _learner(usim, seed=1, n_epochs=10, batch_size=ROWS, learning_rate=1e-3)     # the whole buffer as the minibatch: first and last are the same rows
    out = full.train()
    assert out["bc/action_mse"] < full.first_minibatch["bc/action_mse"] and out["bc/loss"] < full.first_minibatch["bc/loss"]
    _, nov = _learner(usim, seed=1, valued=False)                           # vf_coef 0.5 over a buffer without value targets: no value term, no error
    assert nov.train()["bc/value_loss"] == 0.0 and nov.batch_size is None and int(nov.step_count.item()) == 300 // (300 // 8) + 1


def test_the_same_seed_gives_the_same_parameters(usim):
    thetas = []
    for _ in range(2):
        _, bc = _learner(usim, seed=7, n_epochs=2)
        bc.train(); bc.train()
        torch.cuda.synchronize()
        thetas.append(bc.theta.clone())
    assert torch.equal(thetas[0].view(torch.int32), thetas[1].view(torch.int32)) and torch.isfinite(thetas[0]).all()
    _, other = _learner(usim, seed=8, n_epochs=2)
    other.train()
    assert not torch.equal(other.theta, thetas[0])


def test_native_ppo_built_afterwards_trains_the_same_words(usim):
    _, bc = _learner(usim, seed=2)
    bc.train()
    env = SimpleNamespace(action_dim=A, device=torch.device(DEV), num_envs=8)
    buffer = SimpleNamespace(device=DEV, buffer_size=8, n_envs=8)
    ppo = usim.ppo.NativePPO(env, bc.policy, bc.vecnorm, buffer)
    assert ppo.theta is bc.theta and ppo.theta.data_ptr() == bc.theta.data_ptr() and ppo.params == bc.params
    assert ppo._net.pi_w1 == bc._net.pi_w1 == bc.theta.data_ptr() and ppo._net.log_std == bc._net.log_std
