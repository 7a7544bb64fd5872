"""monitor.evaluate_policy against SB3's own bookkeeping (tests/monitor_ref.py sb3_evaluate_bookkeeping): 64 rigid-torso environments, horizon 12, a
random-initialised MlpActorCritic.  The reference run is a plain Python loop over a second env with the same seed and the same act(), reading done, episode_return
and episode_length to the host after every step."""
import numpy as np
import pytest
import torch

import monitor_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HORIZON = 64, 12


def _setup(usim):
    pol = usim.policy
    kw = usim.default_robosuite_kwargs()
    kw["horizon"] = HORIZON
    env = usim.UltrasoundVecEnv(N, device=DEV, seed=3, torso="rigid", **kw)
    torch.manual_seed(0)
    policy = pol.MlpActorCritic(19, env.action_dim).to(env.device)
    vn = pol.DeviceVecNormalize(N, 19, device=env.device, training=True, norm_reward=True)
    g = torch.Generator().manual_seed(1)                              # statistics that are not the initial ones
    vn.obs_mean.copy_(0.1 * torch.randn(19, generator=g, dtype=torch.float64)); vn.obs_var.copy_(0.5 + torch.rand(19, generator=g, dtype=torch.float64))
    return env, policy, vn


@pytest.fixture(scope="module")
def recorded(usim):
    """(done, episode_return, episode_length) of 3 x HORIZON steps of the deterministic policy, step by step on the host: enough for two episodes per environment"""
    pol = usim.policy
    env, policy, vn = _setup(usim)
    fr = pol.FusedRollout(env, policy, vn, pol.DeviceRolloutBuffer(1, N, 19, env.action_dim, device=env.device), seed=0, graph=False, init_stats=False)
    obs = env.reset_tensor()
    fr.pack()
    steps = []
    for k in range(3 * HORIZON):
        act, _ = fr.act(obs, None, counter=k, training=0, deterministic=True, pack=False)
        obs, _, done = env.step_tensor(act)
        steps.append((done.cpu().numpy().copy(), env.episode_return.cpu().numpy().copy(), env.episode_length.cpu().numpy().copy()))
    env.close()
    return steps


@pytest.mark.parametrize("n_eval", [1, 64, 100])
def test_episode_lists_equal_sb3_bookkeeping(usim, recorded, n_eval):
    env, policy, vn = _setup(usim)
    stats = [t.clone() for t in (vn.obs_mean, vn.obs_var, vn._obs_count, vn.ret_mean, vn.ret_var, vn._ret_count)]
    earlier = env.attach_monitor(usim.DeviceMonitor(env, window=7))
    earlier.block[16:20] = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=DEV)      # a block that is not empty: it must come back untouched
    kept = earlier.block.clone()
    want_r, want_l = ref.sb3_evaluate_bookkeeping(recorded, N, n_eval)
    got_r, got_l = usim.evaluate_policy(env, policy, vn, n_eval_episodes=n_eval, check_every=5, return_episode_rewards=True)
    assert len(want_r) == n_eval and got_r == want_r and got_l == want_l
    assert env.monitor is earlier and torch.equal(earlier.block, kept)
    env.seed(3)                                                       # a reset starts NEW episodes (the draws are keyed on the episode counter): back to the recorded ones
    mean, std = usim.evaluate_policy(env, policy, vn, n_eval_episodes=n_eval)           # the default check_every: the loop runs past the last episode
    assert mean == float(np.mean(want_r)) and std == float(np.std(want_r))
    assert env.monitor is earlier and torch.equal(earlier.block, kept)
    for t, k in zip((vn.obs_mean, vn.obs_var, vn._obs_count, vn.ret_mean, vn.ret_var, vn._ret_count), stats):
        assert torch.equal(t, k)                                      # the statistics are frozen during an evaluation
    env.detach_monitor()
    env.seed(3)
    assert usim.evaluate_policy(env, policy, vn, n_eval_episodes=n_eval) == (mean, std) and env.monitor is None
    env.close()
