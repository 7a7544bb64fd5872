"""ppo.NativePPO.learn keeps a training log: one dict of SB3's logger scalars per iteration in `history`, with the attached monitor's summary and
train/explained_variance (usim_explained_variance on the buffer, before the first minibatch).  64 rigid-torso environments x 16 steps, horizon 8 without early
termination.  The log and the monitor do not touch the training: the parameters after two iterations are those of a run without a monitor, bit for bit."""
import math

import pytest
import torch

import monitor_ref as ref

pytestmark = pytest.mark.gpu
N, T, HORIZON = 64, 16, 8


def _learn(usim, monitored, iterations=2):
    pol, ppo = usim.policy, usim.ppo
    kw = usim.default_robosuite_kwargs()
    kw["horizon"], kw["early_termination"] = HORIZON, False
    env = usim.UltrasoundVecEnv(N, device="cuda:0", seed=3, torso="rigid", **kw)
    dev = env.device
    torch.manual_seed(0)
    policy = pol.MlpActorCritic(19, env.action_dim).to(dev)
    theta = ppo.flatten_parameters(policy)
    vn = pol.DeviceVecNormalize(N, 19, device=dev, training=True, norm_reward=True)
    buf = pol.DeviceRolloutBuffer(T, N, 19, env.action_dim, device=dev)
    mon = env.attach_monitor(usim.DeviceMonitor(env)) if monitored else None      # before the collector is built
    coll = pol.FusedRollout(env, policy, vn, buf, seed=0)
    learner = ppo.NativePPO(env, policy, vn, buf, coll, n_epochs=2, seed=0)
    assert learner.history == []
    out = learner.learn(iterations)
    torch.cuda.synchronize()
    res = dict(history=list(learner.history), out=out, theta=theta.clone(), values=buf.values.clone(), returns=buf.returns.clone(), mon=mon)
    env.close()
    return res


@pytest.fixture(scope="module")
def runs(usim):
    return {True: _learn(usim, True), False: _learn(usim, False)}


def test_history_rows(usim, runs):
    h = runs[True]["history"]
    assert len(h) == 2 and [r["time/total_timesteps"] for r in h] == [N * T, 2 * N * T] == [1024, 2048]
    for r in h:
        assert set(usim.ppo.STAT_NAMES) <= set(r) and {"time/wall", "train/learning_rate", "train/explained_variance"} <= set(r)
        assert r["train/learning_rate"] == pytest.approx(3e-4) and math.isfinite(r["train/loss"])
        assert {"rollout/ep_rew_mean", "rollout/ep_len_mean", "rollout/episodes", "rollout/truncated", "rollout/ep_rew_mean_all", "rollout/ep_len_mean_all"} <= set(r)
        assert r["rollout/ep_len_mean"] == HORIZON and math.isfinite(r["rollout/ep_rew_mean"])
    assert h[0]["time/wall"] <= h[1]["time/wall"]
    assert [r["rollout/episodes"] for r in h] == [N * T // HORIZON, 2 * N * T // HORIZON]      # cumulative
    assert runs[True]["out"] == {k: h[-1][k] for k in usim.ppo.STAT_NAMES}                    # learn() still returns the last update's statistics


def test_explained_variance_of_the_last_row(runs):
    """the buffer is not written between the last update() and the end of learn(): its values / returns are what usim_explained_variance read"""
    for monitored in (True, False):
        r = runs[monitored]
        want = ref.explained_variance(r["values"].cpu().numpy(), r["returns"].cpu().numpy())
        got = r["history"][-1]["train/explained_variance"]
        print(f"explained variance: device {got!r} float64 {want!r}")
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want))


def test_without_a_monitor_no_rollout_keys_and_the_same_parameters(runs):
    plain, monitored = runs[False], runs[True]
    assert len(plain["history"]) == 2 and not any(k.startswith("rollout/") for r in plain["history"] for k in r)
    assert torch.equal(plain["theta"], monitored["theta"])                       # bit for bit
    for a, b in zip(plain["history"], monitored["history"]):
        assert all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a if k != "time/wall")
