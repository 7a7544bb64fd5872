"""evaluation.evaluate_episodes: monitor.evaluate_policy's episodes with their error metrics.  Environments built alike (32 environments, horizon 40, seed 3, a
seeded random MlpActorCritic, statistics that are not the initial ones) play the same episodes, so three of them are compared: evaluate_episodes on one,
evaluate_policy on the second, and on the third a hand-rolled loop of the same act() with error_metrics.DeviceErrorMetrics updated by hand and SB3's bookkeeping
(environment i contributes its first (48 + i) // 32 episodes, a step's episodes in ascending index) applied on the host.

The metrics agree within 1e-12 relative: both sides add the same float64 terms step by step in the same order and divide by the horizon, and differ only inside a
term (fused multiply-adds, torch's norm against an explicit square root) -- an ulp or two of 2.2e-16 on sums of at most 40 terms."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HORIZON, N_EVAL = 32, 40, 48


def _setup(usim, n=N, horizon=HORIZON, **kw_extra):
    pol = usim.policy
    kw = usim.default_robosuite_kwargs()
    kw["horizon"] = horizon
    kw.update(kw_extra)
    env = usim.UltrasoundVecEnv(n, device=DEV, seed=3, **kw)
    torch.manual_seed(0)
    policy = pol.MlpActorCritic(19, env.action_dim).to(env.device)
    vn = pol.DeviceVecNormalize(n, 19, device=env.device, training=True, norm_reward=True)
    g = torch.Generator().manual_seed(1)
    vn.obs_mean.copy_(0.1 * torch.randn(19, generator=g, dtype=torch.float64)); vn.obs_var.copy_(0.5 + torch.rand(19, generator=g, dtype=torch.float64))
    return env, policy, vn


@pytest.fixture(scope="module")
def by_hand(usim):
    """the twin loop: [(environment, step, the 13 metrics of DeviceErrorMetrics.last at that step)] in SB3's order"""
    pol = usim.policy
    env, policy, vn = _setup(usim)
    fr = pol.FusedRollout(env, policy, vn, pol.DeviceRolloutBuffer(1, N, 19, env.action_dim, device=env.device), seed=0, graph=False, init_stats=False)
    em = usim.error_metrics.DeviceErrorMetrics(env)
    obs = env.reset_tensor()
    fr.pack()
    targets = np.array([(N_EVAL + i) // N for i in range(N)])
    counts, out = np.zeros(N, dtype=int), []
    for k in range(int(targets.max()) * HORIZON):
        act, _ = fr.act(obs, None, counter=k, training=0, deterministic=True, pack=False)
        obs, _, done = env.step_tensor(act)
        em.update(done)
        d, last = done.cpu().numpy(), em.last.cpu().numpy()
        for i in range(N):
            if counts[i] < targets[i] and d[i]:
                out.append((i, k, last[i].copy()))
                counts[i] += 1
        if (counts >= targets).all():
            break
    env.close()
    assert len(out) == N_EVAL
    return out


def test_returns_lengths_and_metrics_of_the_episodes_evaluate_policy_counts(usim, by_hand):
    env, policy, vn = _setup(usim)
    twin, policy_b, vn_b = _setup(usim)
    # a monitor and an observer that are attached beforehand: back afterwards, untouched
    earlier = env.attach_monitor(usim.DeviceMonitor(env, window=7))
    earlier.block[16:20] = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=DEV)
    watcher = env.attach_observer(usim.DeviceEpisodeMetrics(env, window=5))
    watcher.block[64:68] = torch.tensor([5, 6, 7, 8], dtype=torch.int32, device=DEV)
    kept_m, kept_w = earlier.block.clone(), watcher.block.clone()
    stats = [t.clone() for t in (vn.obs_mean, vn.obs_var, vn._obs_count, vn.ret_mean, vn.ret_var, vn._ret_count)]

    res = usim.evaluate_episodes(env, policy, vn, n_eval_episodes=N_EVAL, check_every=7, record_envs=[3, 20], record_episodes=1)
    want_r, want_l = usim.evaluate_policy(twin, policy_b, vn_b, n_eval_episodes=N_EVAL, return_episode_rewards=True)

    assert res["returns"].dtype == np.float64 and res["lengths"].dtype == np.int64
    assert res["returns"].tolist() == want_r and res["lengths"].tolist() == want_l and len(want_r) == N_EVAL
    assert res["mean"] == float(np.mean(res["returns"])) and res["std"] == float(np.std(res["returns"]))
    assert list(res["metrics"]) == list(usim.error_metrics.METRICS)
    got = np.stack([res["metrics"][k] for k in usim.error_metrics.METRICS], axis=1)
    want = np.stack([m for _, _, m in by_hand])
    assert got.shape == want.shape == (N_EVAL, 13) and np.isfinite(got).all()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"largest relative difference to DeviceErrorMetrics.last: {rel[want != 0].max():.3e} (bound 1e-12)")
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    rec = res["recorder"]
    assert rec.complete() and [(e["env"], e["index"]) for e in rec.episodes()] == [(3, 0), (20, 0)]
    first = {i: l for (i, _, _), l in zip(reversed(by_hand), reversed(want_l))}               # environment -> length of its FIRST counted episode
    assert [e["length"] for e in rec.episodes()] == [first[3], first[20]]

    assert env.monitor is earlier and env.observers == (watcher,)
    assert torch.equal(earlier.block, kept_m) and torch.equal(watcher.block, kept_w)
    for t, k in zip((vn.obs_mean, vn.obs_var, vn._obs_count, vn.ret_mean, vn.ret_var, vn._ret_count), stats):
        assert torch.equal(t, k)                                      # the statistics are frozen during an evaluation
    env.close(); twin.close()


def test_step_log_is_left_as_it_was(usim):
    env, policy, vn = _setup(usim, n=8, horizon=6, torso="rigid")
    assert env.step_log is None
    res = usim.evaluate_episodes(env, policy, vn, n_eval_episodes=3)
    assert env.step_log is None and env.observers == () and env.monitor is None and res["recorder"] is None and len(res["returns"]) == 3
    env.close()


def _collect_twice(usim, graph):
    pol = usim.policy
    env, policy, vn = _setup(usim, horizon=8, early_termination=False)
    buf = pol.DeviceRolloutBuffer(16, N, 19, env.action_dim, device=env.device)
    met = env.attach_observer(usim.DeviceEpisodeMetrics(env, window=50))          # before the collector is built
    rec = env.attach_observer(usim.EpisodeRecorder(env, [1, 30], episodes=3))
    coll = pol.FusedRollout(env, policy, vn, buf, seed=0, graph=graph)
    for _ in range(2):
        coll.collect()
    torch.cuda.synchronize()
    out = dict(metrics=met.block.cpu().numpy().copy(), record=rec.block.cpu().numpy().copy(), episodes=met.episodes(), summary=met.summary(),
               complete=rec.complete())
    env.close()
    return out


def test_recorded_rollout_feeds_the_observers_like_the_eager_one(usim):
    g, e = _collect_twice(usim, True), _collect_twice(usim, False)
    np.testing.assert_array_equal(g["metrics"], e["metrics"])        # bit for bit
    np.testing.assert_array_equal(g["record"], e["record"])
    s = g["summary"]
    assert s["eval/episodes"] == N * 2 * 16 // 8 == 128 and s["eval/nonfinite"] == 0 and s["eval/mean_ep_length"] == 8 == s["eval/mean_ep_length_all"]
    assert len(g["episodes"]) == 50 and [x["env"] for x in g["episodes"][-N:]] == list(range(N)) and g["complete"]
    names = usim.error_metrics.METRICS
    assert all(np.isfinite(s[f"eval/{k}"]) and np.isfinite(s[f"eval/{k}_all"]) and s[f"eval/{k}_std_all"] >= 0 for k in names)
    assert s["eval/force_mse"] == pytest.approx(np.mean([x["force_mse"] for x in g["episodes"]]), rel=1e-13)          # the same 50 numbers; 50 additions x 2^-53
