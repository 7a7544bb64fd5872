"""population.PopulationPPO(concurrent=True) end to end, on the shapes of tests/test_gpu_population_ppo.py (K = 3, G = 32, T = 8, two epochs of 96-row minibatches:
two full ones and a trailing one of 64 per epoch) with per-member learning rates, entropy coefficients and target_kl: the K updates run as ONE chain of launches
(usim_ppo_grad_multi / usim_ppo_adam_multi) and must compute, bit for bit, what three lone ppo.NativePPO.learn(2) compute on shard environments -- and what the
sequential path computes when the two paths, and a member's lone update(), alternate mid-run."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, G, T, ENV_SEED, NOISE_SEED = 3, 32, 8, 3, 5
SEEDS, RATES, ENT, KL = [11, 12, 13], [3e-4, 1e-3, 3e-4], [0.0, 1e-3, 0.0], [None, 1e-9, None]
HYPER = dict(n_epochs=2, batch_size=96)


def _policies(usim):
    torch.manual_seed(23)
    return [usim.policy.MlpActorCritic(19, 6) for _ in range(K)]


def _env(usim, n, offset=0):
    return usim.UltrasoundVecEnv(n, device=DEV, seed=ENV_SEED, env_offset=offset, **usim.default_robosuite_kwargs())


def _same_number(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _i32(t):
    return t.contiguous().view(torch.int32)


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
        ppo = usim.ppo.NativePPO(env, policy, vn, buf, fr, seed=SEEDS[k], learning_rate=RATES[k], ent_coef=ENT[k], target_kl=KL[k], **HYPER)
        ppo.learn(2)
        torch.cuda.synchronize()
        out.append(dict(theta=theta.clone(), m=ppo.exp_avg.clone(), v=ppo.exp_avg_sq.clone(), steps=int(ppo.step_count.item()), history=ppo.history))
        env.close()
    return out


def _population(usim, concurrent):
    P, M = usim.policy, usim.population
    env = _env(usim, K * G)
    pop = M.PolicyPopulation.from_policies(_policies(usim), device=DEV)
    vn = M.PopulationVecNormalize(K, G, device=DEV)
    buf = P.DeviceRolloutBuffer(T, K * G, 19, env.action_dim, device=DEV)
    coll = M.PopulationRollout(env, pop, vn, buf, seed=NOISE_SEED)
    ppo = M.PopulationPPO(env, pop, vn, buf, coll, seeds=SEEDS, learning_rate=RATES, ent_coef=ENT, target_kl=KL, concurrent=concurrent, **HYPER)
    return env, pop, vn, coll, ppo


def test_concurrent_population_equals_the_lone_learners(usim, lone, tmp_path):
    M = usim.population
    env, pop, vn, coll, ppo = _population(usim, True)
    P_ = pop.params
    # the population owns the learners' state: every learner's tensors are views of its row
    assert ppo.exp_avg.shape == ppo.exp_avg_sq.shape == ppo.grad.shape == (K, pop.stride) and ppo.step_count.shape == (K,) and ppo.gate.shape == (K, 4)
    for k, l in enumerate(ppo.learners):
        for name in ("grad", "exp_avg", "exp_avg_sq"):
            assert getattr(l, name).data_ptr() == getattr(ppo, name)[k].data_ptr() and getattr(l, name).numel() == P_, name
        assert l.step_count.data_ptr() == ppo.step_count[k].data_ptr() and l.stats.data_ptr() == ppo.stats[k].data_ptr() and l.gate.data_ptr() == ppo.gate[k].data_ptr()
        assert l.theta.data_ptr() == pop.theta[k].data_ptr()
    last = ppo.learn(2)
    torch.cuda.synchronize()
    assert len(last) == K
    for k, l in enumerate(ppo.learners):
        want = lone[k]
        assert torch.equal(_i32(l.theta), _i32(want["theta"])), f"member {k}: parameters"
        assert torch.equal(_i32(l.exp_avg), _i32(want["m"])) and torch.equal(_i32(l.exp_avg_sq), _i32(want["v"])), f"member {k}: Adam moments"
        assert int(l.step_count.item()) == want["steps"], f"member {k}: step count"
        assert len(ppo.history[k]) == 2
        for row, ref in zip(ppo.history[k], want["history"]):
            keys = [key for key in ref if key.startswith("train/")]
            assert len(keys) >= 13 and {"train/early_stop", "train/optimizer_steps", "train/std", "train/explained_variance"} <= set(keys)
            assert row["time/total_timesteps"] == ref["time/total_timesteps"]
            for key in keys:
                assert _same_number(row[key], ref[key]), f"member {k}: {key} {row[key]!r} against {ref[key]!r}"
        assert all(_same_number(last[k][key], want["history"][-1][key]) for key in last[k])
    # the cases are what they are meant to be: member 1 stopped early (target_kl 1e-9), the others took every step
    assert [lone[k]["steps"] for k in (0, 2)] == [2 * 2 * 3] * 2 and lone[1]["steps"] < 2 * 2 * 3
    assert ppo.history[1][-1]["train/early_stop"] == 1 and ppo.history[0][-1]["train/early_stop"] == 0
    # the collector's packed weights are those of the updated parameters
    packed = pop.packed.clone()
    pop.pack()
    torch.cuda.synchronize()
    assert torch.equal(packed, pop.packed)
    # one checkpoint pair per member through the existing writers, and back into the population's rows
    paths = ppo.save_checkpoint(tmp_path, [f"member_{k}" for k in range(K)])
    again = M.PolicyPopulation.from_checkpoints([z for z, _ in paths], device=DEV)
    assert torch.equal(again.theta[:, :P_], pop.theta[:, :P_])
    m1, v1, ptr = ppo.exp_avg.clone(), ppo.exp_avg_sq.clone(), ppo.learners[1].exp_avg.data_ptr()
    ppo.exp_avg.zero_(); ppo.exp_avg_sq.zero_(); ppo.step_count.zero_()
    for k, l in enumerate(ppo.learners):
        l.load_checkpoint(tmp_path, f"member_{k}")
    torch.cuda.synchronize()
    assert torch.equal(_i32(ppo.exp_avg[:, :P_]), _i32(m1[:, :P_])) and torch.equal(_i32(ppo.exp_avg_sq[:, :P_]), _i32(v1[:, :P_]))
    assert ppo.step_count.tolist() == [lone[k]["steps"] for k in range(K)] and ppo.learners[1].exp_avg.data_ptr() == ptr
    env.close()


def test_the_paths_alternate_mid_run(usim):
    """iteration 1 concurrent, iteration 2 every member's lone update(), iteration 3 concurrent again = three iterations of the sequential path"""
    env_a, pop_a, _, coll_a, a = _population(usim, True)
    env_b, pop_b, _, coll_b, b = _population(usim, False)
    out_a, out_b = [], []
    for it in range(3):
        coll_a.collect()
        if it == 1:
            out_a.append([l.update() for l in a.learners])
            coll_a.pack()
        else:
            out_a.append(a.update())
        coll_b.collect()
        out_b.append(b.update())
    torch.cuda.synchronize()
    assert torch.equal(_i32(pop_a.theta), _i32(pop_b.theta)) and torch.equal(pop_a.packed, pop_b.packed)
    for k in range(K):
        la, lb = a.learners[k], b.learners[k]
        assert torch.equal(_i32(la.exp_avg), _i32(lb.exp_avg)) and torch.equal(_i32(la.exp_avg_sq), _i32(lb.exp_avg_sq)) and int(la.step_count.item()) == int(lb.step_count.item())
        assert torch.equal(_i32(la.first_stats), _i32(lb.first_stats))
        for it in range(3):
            assert all(_same_number(out_a[it][k][key], out_b[it][k][key]) for key in out_b[it][k]), (it, k)
        assert la.last_update == lb.last_update
    env_a.close(); env_b.close()
