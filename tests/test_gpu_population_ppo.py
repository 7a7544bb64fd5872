"""population.PopulationPPO against its oracle: K = 3 members trained side by side over one PopulationRollout (per-member shuffle seeds, two different learning
rates) must compute, bit for bit, what three lone ppo.NativePPO.learn(2) runs compute over shard environments (num_envs = G, env_offset = k G, same seed) and
their lone policy.FusedRollout(fused_stats=False): every member's parameters, Adam moments and train/* rows.  G = 32, T = 8, the `tracking` defaults."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, G, T, ENV_SEED, NOISE_SEED = 3, 32, 8, 3, 5
SEEDS, RATES = [11, 12, 13], [3e-4, 1e-3, 3e-4]
HYPER = dict(n_epochs=2, batch_size=96)                                    # 256 rows per member: two full minibatches and a trailing one of 64 per epoch


def _policies(usim):
    torch.manual_seed(23)
    return [usim.policy.MlpActorCritic(19, 6) for _ in range(K)]


def _env(usim, n, offset=0):
    return usim.UltrasoundVecEnv(n, device=DEV, seed=ENV_SEED, env_offset=offset, **usim.default_robosuite_kwargs())


def _same_number(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.fixture(scope="module")
def lone(usim):
    P, out = usim.policy, []
    for k, src in enumerate(_policies(usim)):
        env = _env(usim, G, offset=k * G)
        policy = src.to(DEV)
        theta = usim.ppo.flatten_parameters(policy)
        vn = P.DeviceVecNormalize(G, device=DEV)
        buf = P.DeviceRolloutBuffer(T, G, 19, env.action_dim, device=DEV)
        fr = P.FusedRollout(env, policy, vn, buf, seed=NOISE_SEED, fused_stats=False)
        ppo = usim.ppo.NativePPO(env, policy, vn, buf, fr, seed=SEEDS[k], learning_rate=RATES[k], **HYPER)
        last = ppo.learn(2)
        torch.cuda.synchronize()
        out.append(dict(theta=theta.clone(), m=ppo.exp_avg.clone(), v=ppo.exp_avg_sq.clone(), steps=int(ppo.step_count.item()), history=ppo.history, last=last,
                        obs_mean=vn.obs_mean.clone()))
        env.close()
    return out


def test_population_ppo_equals_the_lone_learners(usim, lone, tmp_path):
    P, M = usim.policy, usim.population
    env = _env(usim, K * G)
    pop = M.PolicyPopulation.from_policies(_policies(usim), device=DEV)
    vn = M.PopulationVecNormalize(K, G, device=DEV)
    buf = P.DeviceRolloutBuffer(T, K * G, 19, env.action_dim, device=DEV)
    coll = M.PopulationRollout(env, pop, vn, buf, seed=NOISE_SEED)
    ppo = M.PopulationPPO(env, pop, vn, buf, coll, seeds=SEEDS, learning_rate=RATES, **HYPER)
    theta0 = pop.theta.clone()
    last = ppo.learn(2)
    torch.cuda.synchronize()
    assert len(ppo.learners) == K and len(ppo.history) == K and len(last) == K
    for k, l in enumerate(ppo.learners):
        want = lone[k]
        assert l.theta.data_ptr() == pop.theta[k].data_ptr() and l.buffer.n_envs == G and l.rollout == T * G
        assert torch.equal(l.theta.view(torch.int32), want["theta"].view(torch.int32)), f"member {k}: parameters"
        assert torch.equal(l.exp_avg.view(torch.int32), want["m"].view(torch.int32)) and torch.equal(l.exp_avg_sq.view(torch.int32), want["v"].view(torch.int32)), f"member {k}: Adam moments"
        assert int(l.step_count.item()) == want["steps"] == 2 * 2 * 3
        assert torch.equal(vn.member(k).obs_mean, want["obs_mean"])
        assert len(ppo.history[k]) == 2
        for row, ref in zip(ppo.history[k], want["history"]):
            keys = [key for key in ref if key.startswith("train/")]
            assert len(keys) >= 8 and row["time/total_timesteps"] == ref["time/total_timesteps"]
            for key in keys:
                assert _same_number(row[key], ref[key]), f"member {k}: {key} {row[key]!r} against {ref[key]!r}"
        assert all(_same_number(last[k][key], want["last"][key]) for key in want["last"])
        assert not torch.equal(pop.theta[k], theta0[k])                    # the member learned something
    assert ppo.history[1][0]["train/learning_rate"] == 1e-3 and ppo.history[0][0]["train/learning_rate"] == 3e-4
    # the collector's packed weights are those of the updated parameters
    packed = pop.packed.clone()
    pop.pack()
    torch.cuda.synchronize()
    assert torch.equal(packed, pop.packed)
    # one checkpoint pair per member, through the existing writers
    names = [f"member_{k}" for k in range(K)]
    paths = ppo.save_checkpoint(tmp_path, names)
    again = M.PolicyPopulation.from_checkpoints([z for z, _ in paths], device=DEV)
    assert torch.equal(again.theta[:, :pop.params], pop.theta[:, :pop.params])
    st = P.load_vecnormalize_pkl(paths[2][1])
    assert torch.equal(torch.as_tensor(st["obs_mean"]), vn.member(2).obs_mean.cpu()) and st["count"] == vn.member(2).obs_count
    env.close()
