"""tests/bootstrap_ref.py, the float64 restatement of usim_policy_bootstrap, against a literal transcription of stable-baselines3's loop, and the torch
branch of policy._rollout_step (collect_rollouts / GraphedCollector with bootstrap_truncation=True) on CPU tensors against the restatement.  No GPU."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bootstrap_ref as B
import policy_ref as R

ROOT = Path(__file__).resolve().parent.parent
GAMMA = float(np.float32(0.99))


def _params(weights):
    if weights == "tracking":
        return {k: np.asarray(v, dtype=np.float32) for k, v in R.params_from_sb3(dict(np.load(ROOT / "tests/golden/tracking_policy.npz"))).items()}
    return B.orthogonal_params(5)


def _module(usim, p, dtype):
    m = usim.policy.MlpActorCritic(19, p["act_b"].shape[0])
    names = {"pi_w1": m.policy_net[0].weight, "pi_b1": m.policy_net[0].bias, "pi_w2": m.policy_net[2].weight, "pi_b2": m.policy_net[2].bias,
             "act_w": m.action_net.weight, "act_b": m.action_net.bias, "vf_w1": m.value_net_body[0].weight, "vf_b1": m.value_net_body[0].bias,
             "vf_w2": m.value_net_body[2].weight, "vf_b2": m.value_net_body[2].bias, "val_w": m.value_net.weight, "val_b": m.value_net.bias, "log_std": m.log_std}
    with torch.no_grad():
        for k, t in names.items():
            t.copy_(torch.from_numpy(np.asarray(p[k])))
    return m.to(dtype)


@pytest.mark.parametrize("weights", ["tracking", "orthogonal"])
@pytest.mark.parametrize("pattern", B.PATTERNS)
def test_restatement_equals_sb3_loop(usim, weights, pattern):
    """OnPolicyAlgorithm.collect_rollouts: for idx, done in enumerate(dones): if done and infos[idx].get("terminal_observation") is not None and
    infos[idx].get("TimeLimit.truncated", False): rewards[idx] += gamma * policy.predict_values(obs_as_tensor(terminal_obs))[0] -- with the infos of the
    numpy path (terminal_observation normalised by VecNormalize.step_wait -> float32; TimeLimit.truncated = ep_length >= horizon) and a float64 policy"""
    rng = np.random.default_rng(B.PATTERNS.index(pattern))
    n, p = 70, _params(weights)
    policy = _module(usim, p, torch.float64)
    mean, var = B.crafted_stats(rng)
    done, ep = B.crafted_flags(rng, n, pattern)
    tr = B.truncated(done, ep, B.HORIZON)
    term = B.poison(B.crafted_obs(rng, n, mean, var), tr)
    rew = (rng.normal(size=n) * 3).astype(np.float32)
    out, bound, tr2, value, _ = B.bootstrap(p, mean, var, term, done, ep, B.HORIZON, GAMMA, rew)
    rewards = rew.astype(np.float64)
    for idx in range(n):
        info = {}
        if done[idx]:
            nobs = np.clip((term[idx] - mean) / np.sqrt(var + 1e-8), -10.0, 10.0).astype(np.float32)          # VecNormalize.normalize_obs
            info = {"terminal_observation": nobs, "TimeLimit.truncated": bool(ep[idx] >= B.HORIZON)}
        if done[idx] and info.get("terminal_observation") is not None and info.get("TimeLimit.truncated", False):
            with torch.no_grad():
                terminal_value = policy.forward(torch.from_numpy(info["terminal_observation"]).to(torch.float64)[None])[1][0]
            rewards[idx] += GAMMA * float(terminal_value)
    assert np.array_equal(tr, tr2) and tr.sum() == {"none": 0, "all": n, "last": 1, "alternating": 35, "early": 0, "stale": 0}.get(pattern, tr.sum())
    assert np.array_equal(out[~tr], rew[~tr].astype(np.float64)) and np.all(bound[~tr] == 0)
    assert np.all(np.abs(out - rewards) <= 1e-10), np.abs(out - rewards).max()
    assert np.all(np.isfinite(out)) and (pattern == "all" or np.isnan(term).any())
    if tr.any():
        assert np.all(bound[tr] > 0) and np.all(bound[tr] < 1e-3 * (1 + np.abs(out[tr])))                      # (a bound, not a tolerance: parts per million)
        nobs = B.normalize(term[tr], mean, var)
        assert (nobs == 10).any() or (nobs == -10).any() or tr.sum() < 3


class _Env:
    """the four things _rollout_step asks of an environment, on CPU tensors: one crafted step"""

    def __init__(self, obs, rew, done, term, ep, horizon):
        self._out = (torch.from_numpy(obs), torch.from_numpy(rew), torch.from_numpy(done))
        self.terminal_obs, self._ep, self.horizon = torch.from_numpy(term), torch.from_numpy(ep), horizon

    def step_tensor(self, act):
        return self._out

    @property
    def truncated(self):
        return self._out[2].bool() & (self._ep >= self.horizon)


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("weights", ["tracking", "orthogonal"])
def test_torch_branch_on_cpu_tensors(usim, weights, training):
    pol = usim.policy
    p = _params(weights)
    policy = _module(usim, p, torch.float32)
    low, high = -torch.ones(6), torch.ones(6)
    worst = 0.0
    for k, pattern in enumerate(B.PATTERNS):
        rng = np.random.default_rng(100 + k)
        n = 70
        mean, var = B.crafted_stats(rng)
        done, ep = B.crafted_flags(rng, n, pattern)
        tr = B.truncated(done, ep, B.HORIZON)
        term = B.poison(B.crafted_obs(rng, n, mean, var), tr)
        obs0, obs1 = B.crafted_obs(rng, n, mean, var), B.crafted_obs(rng, n, mean, var)
        rew = (rng.normal(size=n) * 3).astype(np.float32)

        def vecnorm():
            stats = dict(obs_mean=mean, obs_var=var, count=500.0, ret_mean=0.0, ret_var=4.0, ret_count=500.0, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
            return pol.DeviceVecNormalize.from_stats(stats, n, device="cpu", training=training, norm_reward=True)

        vn, twin = vecnorm(), vecnorm()
        stored = {}
        env = _Env(obs1, rew, done, term, ep, B.HORIZON)
        gen = torch.Generator().manual_seed(k)
        o, start, d = pol._rollout_step(env, policy, vn, low, high, torch.from_numpy(obs0), torch.ones(n, dtype=torch.bool), gen,
                                        lambda *a: stored.update(nrew=a[2].clone()), bootstrap_gamma=GAMMA)
        # the statistics are those of a step without the option, bit for bit; the bootstrap saw them with the new observation taken in
        twin.normalize_obs(torch.from_numpy(obs0))
        nrew = twin.normalize_reward(torch.from_numpy(rew), torch.from_numpy(done))
        for name in ("obs_mean", "obs_var", "_obs_count", "ret_mean", "ret_var", "_ret_count", "returns"):
            assert torch.equal(getattr(vn, name), getattr(twin, name)), name
        if training:
            twin._update(twin.obs_mean, twin.obs_var, twin._obs_count, torch.from_numpy(obs1))
        out, bound, _, _, _ = B.bootstrap(p, twin.obs_mean.numpy(), twin.obs_var.numpy(), term, done, ep, B.HORIZON, GAMMA, nrew.numpy(), fused=False)
        got = stored["nrew"].numpy()
        assert got.dtype == np.float32 and np.array_equal(got[~tr].view(np.uint32), nrew.numpy()[~tr].view(np.uint32))      # untouched rows: the same bits, no NaN leaks
        if tr.any():
            err = np.abs(got[tr].astype(np.float64) - out[tr])
            assert np.all(err <= bound[tr]), (pattern, float((err / bound[tr]).max()))
            worst = max(worst, float((err / bound[tr]).max()))
            assert np.all(got[tr] != nrew.numpy()[tr])
        assert torch.equal(o, torch.from_numpy(obs1)) and torch.equal(d, torch.from_numpy(done))
    print(f"\ntorch branch on CPU ({weights}, training={training}): worst error / bound {worst:.3g}")
    assert worst > 0


def test_option_off_is_the_step_as_before(usim):
    """bootstrap_gamma=None: _rollout_step never asks the environment for `truncated` or `terminal_obs`"""
    pol = usim.policy
    policy = _module(usim, _params("orthogonal"), torch.float32)
    rng = np.random.default_rng(1)
    mean, var = B.crafted_stats(rng)
    n = 8
    obs, rew, done = B.crafted_obs(rng, n, mean, var), np.ones(n, np.float32), np.ones(n, np.uint8)
    env = SimpleNamespace(step_tensor=lambda a: (torch.from_numpy(obs), torch.from_numpy(rew), torch.from_numpy(done)))
    vn = pol.DeviceVecNormalize(n, device="cpu")
    stored = {}
    pol._rollout_step(env, policy, vn, -torch.ones(6), torch.ones(6), torch.from_numpy(obs), torch.ones(n, dtype=torch.bool), torch.Generator().manual_seed(0),
                      lambda *a: stored.update(nrew=a[2]))
    assert stored["nrew"].shape == (n,)
