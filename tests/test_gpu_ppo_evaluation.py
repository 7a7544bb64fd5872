"""ppo.NativePPO.set_evaluation: SB3's EvalCallback for learn().  64 rigid-torso environments x 16 steps, horizon 8 without early termination, three iterations,
an evaluation on a second environment after every iteration.  The evaluation reads the live policy and the live statistics and writes neither: the train/* columns
and the parameters are those of a learner without evaluation, bit for bit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
N, T, HORIZON, ITERATIONS, N_EVAL = 64, 16, 8, 3, 10


def _env(usim, n=N, seed=3):
    kw = usim.default_robosuite_kwargs()
    kw["horizon"], kw["early_termination"] = HORIZON, False
    return usim.UltrasoundVecEnv(n, device="cuda:0", seed=seed, torso="rigid", **kw)


def _learn(usim, evaluated):
    pol, ppo = usim.policy, usim.ppo
    env = _env(usim)
    dev = env.device
    torch.manual_seed(0)
    policy = pol.MlpActorCritic(19, env.action_dim).to(dev)
    theta = ppo.flatten_parameters(policy)
    vn = pol.DeviceVecNormalize(N, 19, device=dev, training=True, norm_reward=True)
    buf = pol.DeviceRolloutBuffer(T, N, 19, env.action_dim, device=dev)
    coll = pol.FusedRollout(env, policy, vn, buf, seed=0)
    learner = ppo.NativePPO(env, policy, vn, buf, coll, n_epochs=2, seed=0)
    assert learner.eval_every is None
    other = None
    if evaluated:
        with pytest.raises(ValueError):
            learner.set_evaluation(N * T, eval_env=env)               # the training environment itself
        with pytest.raises(ValueError):
            learner.set_evaluation(N * T)                             # no environment
        with pytest.raises(ValueError):
            learner.set_evaluation(0, eval_env=env)
        assert learner.eval_every is None
        other = _env(usim, seed=5)
        learner.set_evaluation(eval_every=N * T, eval_env=other, n_eval_episodes=N_EVAL)
        other.attach_monitor(usim.DeviceMonitor(other))               # what the evaluation environment carries stays on it
    learner.learn(ITERATIONS)
    torch.cuda.synchronize()
    res = dict(history=list(learner.history), theta=theta.clone(), stats=[t.clone() for t in (vn.obs_mean, vn.obs_var, vn.ret_var)],
               other_monitor=None if other is None else (other.monitor, other.observers, other.step_log))
    if evaluated:
        learner.set_evaluation(None)
        assert learner.eval_every is None and learner.eval_env is None
        other.close()
    env.close()
    return res


@pytest.fixture(scope="module")
def runs(usim):
    return {True: _learn(usim, True), False: _learn(usim, False)}


def test_every_row_has_the_fifteen_eval_scalars(usim, runs):
    h = runs[True]["history"]
    keys = ["eval/mean_reward", "eval/mean_ep_length"] + [f"eval/{k}" for k in usim.error_metrics.METRICS]
    assert len(h) == ITERATIONS and len(keys) == 15
    for r in h:
        assert all(k in r and math.isfinite(r[k]) for k in keys)
        assert sorted(k for k in r if k.startswith("eval/")) == sorted(keys)
        assert r["eval/mean_ep_length"] == HORIZON                    # no early termination: every episode runs to the time limit
    mon, observers, log = runs[True]["other_monitor"]
    assert mon is not None and observers == () and log is None


def test_evaluation_does_not_disturb_training(runs):
    plain, evaluated = runs[False]["history"], runs[True]["history"]
    assert len(plain) == ITERATIONS and not any(k.startswith("eval/") for r in plain for k in r)
    for a, b in zip(plain, evaluated):
        train = [k for k in a if k.startswith("train/")]
        assert len(train) >= 8 and a["time/total_timesteps"] == b["time/total_timesteps"]
        assert all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in train), [(k, a[k], b[k]) for k in train if a[k] != b[k]]
    assert torch.equal(runs[False]["theta"], runs[True]["theta"])     # bit for bit
    for a, b in zip(runs[False]["stats"], runs[True]["stats"]):
        assert torch.equal(a, b)
