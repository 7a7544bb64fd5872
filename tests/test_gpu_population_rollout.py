"""population.PopulationRollout and population.evaluate_population against their oracle: environments do not depend on their neighbours, so a population of K
members over K G environments must compute, bit for bit, what K lone runs compute -- policy.FusedRollout(fused_stats=False) / monitor.evaluate_policy on shard
environments (num_envs = G, env_offset = k G, same seed).  K = 3, G = 32, T = 8, the `tracking` defaults."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, G, T, ENV_SEED, NOISE_SEED = 3, 32, 8, 3, 5
BUFFERS = ("observations", "actions", "values", "log_probs", "rewards", "episode_starts", "advantages", "returns")
STATS = ("obs_mean", "obs_var", "_obs_count", "ret_mean", "ret_var", "_ret_count", "returns")


def _bits(t):
    return t.reshape(-1).contiguous().view(torch.int32).clone()


def _policies(usim):
    torch.manual_seed(17)
    return [usim.policy.MlpActorCritic(19, 6) for _ in range(K)]


def _env(usim, n, offset=0, **over):
    kw = dict(usim.default_robosuite_kwargs(), **over)
    return usim.UltrasoundVecEnv(n, device=DEV, seed=ENV_SEED, env_offset=offset, **kw)


def _snapshot(buffer, vecnorm, cols=slice(None)):
    out = {name: _bits(getattr(buffer, name)[:, cols]) for name in BUFFERS}
    out.update({"stats." + name: _bits(getattr(vecnorm, name)) for name in STATS})
    return out


@pytest.fixture(scope="module")
def lone(usim):
    """the three lone runs, two rollouts each: [k][rollout] -> the buffer and statistics words (+ the raw reward sum)"""
    P = usim.policy
    out = []
    for k, src in enumerate(_policies(usim)):
        env = _env(usim, G, offset=k * G)
        policy = src.to(DEV)
        vn = P.DeviceVecNormalize(G, device=DEV)
        buf = P.DeviceRolloutBuffer(T, G, 19, env.action_dim, device=DEV)
        fr = P.FusedRollout(env, policy, vn, buf, seed=NOISE_SEED, graph=True, fused_stats=False)
        snaps = []
        for _ in range(2):
            fr.collect()
            torch.cuda.synchronize()
            snaps.append(dict(_snapshot(buf, vn), raw=_bits(fr.raw_reward_sum.reshape(1))))
        out.append(snaps)
        env.close()
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_population_rollout_equals_the_lone_runs(usim, lone, graph):
    P, M = usim.policy, usim.population
    env = _env(usim, K * G)
    pop = M.PolicyPopulation.from_policies(_policies(usim), device=DEV)
    vn = M.PopulationVecNormalize(K, G, device=DEV)
    buf = P.DeviceRolloutBuffer(T, K * G, 19, env.action_dim, device=DEV)
    pr = M.PopulationRollout(env, pop, vn, buf, seed=NOISE_SEED, graph=graph)
    assert (pr.graph is not None) == graph
    for r in range(2):
        pr.collect()
        torch.cuda.synchronize()
        assert buf.full
        for k in range(K):
            got = dict(_snapshot(buf, vn.member(k), slice(k * G, (k + 1) * G)), raw=_bits(pr.raw_reward_sum[k:k + 1]))
            for name, want in lone[k][r].items():
                assert torch.equal(got[name], want), f"rollout {r}, member {k}: {name} differs in {int((got[name] != want).sum())} of {want.numel()} words"
    # the members did different things, and the second rollout is not the first again
    assert not torch.equal(lone[0][1]["actions"], lone[1][1]["actions"]) and not torch.equal(lone[0][0]["actions"], lone[0][1]["actions"])
    assert not torch.equal(lone[0][1]["stats.obs_mean"], lone[1][1]["stats.obs_mean"])
    env.close()


def test_evaluate_population_equals_evaluate_policy_on_the_shards(usim):
    P, M = usim.policy, usim.population
    rng = np.random.default_rng(3)
    stats = [dict(obs_mean=0.1 * rng.standard_normal(19), obs_var=0.5 + rng.random(19), count=1000.0 + k, ret_mean=0.1 * k, ret_var=1.0 + k, ret_count=500.0,
                  clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8) for k in range(K)]
    want = []
    for k, src in enumerate(_policies(usim)):
        env = _env(usim, G, offset=k * G, horizon=40)
        vn = P.DeviceVecNormalize.from_stats(stats[k], G, device=DEV)
        want.append(usim.evaluate_policy(env, src.to(DEV), vn, n_eval_episodes=5, return_episode_rewards=True))
        env.close()
    env = _env(usim, K * G, horizon=40)
    pop = M.PolicyPopulation.from_policies(_policies(usim), device=DEV)
    vn = M.PopulationVecNormalize(K, G, device=DEV, training=False, norm_reward=False)
    for k in range(K):
        vn.load_member(k, stats[k])
    kept = vn.obs_mean.clone()
    mon = env.attach_monitor(usim.DeviceMonitor(env))
    got = M.evaluate_population(env, pop, vn, n_eval_episodes=5, return_episode_rewards=True)
    assert env.monitor is mon and mon.episode_count() == 0                  # the monitor attached before is back, untouched
    assert torch.equal(vn.obs_mean, kept)                                   # the statistics are frozen
    assert len(got) == K
    for k in range(K):
        assert len(got[k][0]) == 5 and got[k] == want[k], f"member {k}: {got[k]} against {want[k]}"
    assert got[0] != got[1]
    env.close()
    env = _env(usim, K * G, horizon=40)                                     # (a second evaluation on the same env draws new resets: a fresh one for the same episodes)
    pairs = M.evaluate_population(env, pop, vn, n_eval_episodes=5)
    for k in range(K):
        assert pairs[k] == (float(np.mean(want[k][0])), float(np.std(want[k][0])))
    env.close()
